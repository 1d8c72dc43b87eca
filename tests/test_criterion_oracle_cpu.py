"""CPU: the criterion oracle (tests/criterion_oracle.py) is sound before a GPU is touched -- the float32 emulation of the kernels' roundings
stays under CEILING against the float64 reference over the whole table, its fp32 outputs stay within 1/8 of the tolerances the GPU tests
use, the table reaches every code path of csrc/loss_optim.hip by plain arithmetic on (V, ld), the underflow floor never hides a planted or a
target column, and the table + metric catch each named mutation of the emulation at the tolerance the GPU tests use.
Run with -s for the measured ceilings, the fp32 figures, the per-mutation worst excess and the fp16 floor shares."""
import functools

import pytest
import torch

from tests import criterion_oracle as co

BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
NAMES = {BF16: "bf16", FP16: "fp16", FP32: "fp32"}
ids = lambda dts: [NAMES[d] for d in dts]          # noqa: E731


def grad_excess(got, ref, bd, dtype, g):
    """16-bit: excess in units of the type's eps (limit: CEILING here, TOL on the GPU); fp32: error / bound (limit: G32_TOL / 8 here)."""
    return co.excess(got, ref, bd, co.EPS.get(dtype, 1.0), co.floor_of(dtype, g))


# ------------------------------------------------------------------------------------------------------------------ evaluation per family
def ce_eval(case, dtype, mutation=None):
    b = co.build_ce(case, dtype)
    ref, bd = co.ce_reference(b["x"], b["t"], b["g"])
    em = co.ce_emulate(b["x"], b["t"], b["g"], dtype, case.fused, mutation)
    f32 = dict(lse=float((em["lse"].double() - ref["lse"]).abs().max()), row=float((em["row_loss"].double() - ref["row_loss"]).abs().max()))
    return grad_excess(em["d"], ref["d"], bd, dtype, b["g"]), f32


def ls_eval(case, dtype, mutation=None):
    b = co.build_ls(case, dtype)
    kw = dict(crange=b["crange"], cmask=b["cmask"], row_w=b["row_w"])
    ref, bd = co.lsce_reference(b["x"], b["t"], b["g"], b["eps"], **kw)
    em = co.lsce_emulate(b["x"], b["t"], b["g"], b["eps"], dtype, mutation=mutation, **kw)
    f32 = dict(lse=float((em["lse"].double() - ref["lse"]).abs().max()),
               lsrow=max(float((em[n].double() - ref[n]).abs().max()) for n in ("row_loss", "row_nll")))
    f32["cnt"] = float((em["row_cnt"].double() != ref["row_cnt"]).sum())          # row_cnt equals the reference count exactly
    return grad_excess(em["d"], ref["d"], bd, dtype, b["g"]), f32


def probs_eval(case, dtype, mutation=None):
    b = co.build_probs(case, dtype)
    V = case.V
    y = co.probs_emulate(b["x"], case.log_probs, mutation)
    yerr = float((y.double() - co.probs_reference(b["x"], case.log_probs)).abs().max())
    clean = co.probs_emulate(b["x"], case.log_probs)           # the backward is judged on the forward's own stored result
    ref, bd = co.probs_bwd_reference(b["dy"], clean, co.bwd_ld(V), case.log_probs)
    d = co.probs_bwd_emulate(b["dy"], clean, co.bwd_ld(V), case.log_probs, dtype, mutation)
    return grad_excess(d, ref, bd, dtype, co.PLANT_DY), {("plog" if case.log_probs else "pprob"): yerr}


FAMILIES = {"ce_two": (co.CE_TWO_CASES, ce_eval, co.DTYPES3), "ce_fused": (co.CE_FUSED_CASES, ce_eval, co.CE_DTYPES[True]),
            "lsce": (co.LS_CASES, ls_eval, co.DTYPES3), "probs": (co.P_CASES, probs_eval, co.DTYPES3)}
F32_LIMIT = dict(cnt=0.0, lse=co.LSE_TOL, row=co.ROW_TOL, lsrow=co.LSROW_TOL, plog=co.PROBS_TOL[True], pprob=co.PROBS_TOL[False])


def test_constants_hang_together():
    assert co.TOL == 2 * co.CEILING and co.CEILING <= 1.1
    assert co.EPS == {BF16: 2.0 ** -8, FP16: 2.0 ** -11}


@pytest.mark.parametrize("family,dtype", [(f, d) for f in FAMILIES for d in FAMILIES[f][2]],
                         ids=[f"{f}-{NAMES[d]}" for f in FAMILIES for d in FAMILIES[f][2]])
def test_emulation_stays_within_the_ceiling(family, dtype):
    """excess(emulate, reference, bound) <= CEILING over the family's whole table in each 16-bit type; with fp32 logits the gradient's
    error / bound and every fp32 output's absolute error stay within 1/8 of the tolerances the GPU tests use."""
    cases, fn, _ = FAMILIES[family]
    worst, wcase, w32 = 0.0, None, {}
    for case in cases:
        e, f32 = fn(case, dtype)
        if e > worst:
            worst, wcase = e, case
        for n, v in f32.items():
            w32[n] = max(w32.get(n, 0.0), v)
    print(f"\n{family} {NAMES[dtype]}: worst gradient {'error / bound' if dtype == FP32 else 'excess'} {worst:.3g} at {wcase}; "
          f"fp32 outputs {{{', '.join(f'{n}: {v:.2e}' for n, v in w32.items())}}}")
    if dtype == FP32:
        assert 8 * worst <= co.G32_TOL, (worst, wcase)
    else:
        assert worst <= co.CEILING, (worst, wcase)
    for n, v in w32.items():
        assert 8 * v <= F32_LIMIT[n], (n, v)


# ------------------------------------------------------------------------------------------------------------------ mutations
@functools.lru_cache(maxsize=None)
def _clean(family, case):
    return FAMILIES[family][1](case, BF16)[0]


def _ce_applies(m, case, dtype):
    N, V, ld = co.NVEC[dtype], case.V, case.ld
    if m == "drop_last_col":
        return V > 1
    if m == "drop_tail_vector":
        return 0 < V // N * N < V
    if m == "drop_slab":
        return case.fused and V > 8192
    if m == "onehot_unscaled":
        return case.g != 1.0
    if m == "pad_written":
        return ld > V
    return True


def _ls_applies(m, case, dtype):
    V = case.V
    if m == "range_edge":
        return case.crange is not None and case.crange[1] < V
    if m == "count_off":
        return case.eps > 0
    if m == "drop_trip":
        return V > 256
    if m == "pad_written":
        return co.build_ls(case, dtype)["x"].stride(0) > V
    return True


def _p_applies(m, case, dtype):
    if m == "drop_trip":
        return case.V > 256
    if m == "pad_written":
        return co.bwd_ld(case.V) > case.V
    return case.V > 1


SUM_MUTATIONS = ("drop_last_col", "drop_tail_vector", "drop_slab", "drop_trip")


def _covers(family, case, mutation):
    """Does the mutation drop a column that this (planted) entry plants in a row whose gradient is checked there?"""
    N = 1 if family in ("lsce", "probs") else co.NVEC[BF16]
    V = case.V
    dropped = ~co._kept(V, N, mutation, "cpu")
    if family == "probs":
        return any(bool(dropped[c]) for cs in co.build_probs(case, BF16)["cols"] for c in cs)
    bd, _, keys = _bounds_of(family, case, BF16)
    return any(bool(dropped[c]) and float(bd[r, c]) > 0 for r, c in keys)


MUTANTS = [("ce_two", m, _ce_applies) for m in co.CE_MUTATIONS if m != "drop_slab"] + [("ce_fused", m, _ce_applies) for m in co.CE_MUTATIONS] + \
          [("lsce", m, _ls_applies) for m in co.LSCE_MUTATIONS] + [("probs", m, _p_applies) for m in co.PROBS_MUTATIONS]


@pytest.mark.parametrize("family,mutation,applies", MUTANTS, ids=[f"{f}-{m}" for f, m, _ in MUTANTS])
def test_table_and_metric_catch_the_mutation(family, mutation, applies):
    """Each subtly wrong variant of the emulation exceeds the GPU tolerance TOL (bf16, per element) in at least one table entry it
    applies to, while the unmutated emulation of that entry stays under the ceiling.  A mutation of the sum that covers a planted column
    must be caught in EVERY planted entry it applies to."""
    cases, fn, _ = FAMILIES[family]
    worst, caught, covered, missed_planted = 0.0, 0, 0, []
    for case in cases:
        if not applies(mutation, case, BF16):
            continue
        e, _ = fn(case, BF16, mutation)
        covers = mutation in SUM_MUTATIONS and case.regime == "planted" and _covers(family, case, mutation)
        covered += covers
        if e > co.TOL:
            assert _clean(family, case) <= co.CEILING, case
            caught += 1
        elif covers:
            missed_planted.append((case, e))
        worst = max(worst, e)
    print(f"\n{family} {mutation}: caught in {caught} entries, worst excess {worst:.4g}" +
          (f"; drops a planted column in {covered} planted entries, all caught" if mutation in SUM_MUTATIONS else ""))
    assert caught, f"no table entry notices {mutation}: the table is missing a case"
    if mutation in SUM_MUTATIONS:
        assert covered and not missed_planted, missed_planted


@pytest.mark.parametrize("family,mutation", [("ce_two", "lse_off"), ("ce_fused", "lse_off"), ("lsce", "lse_off"), ("lsce", "count_off")])
def test_fp32_outputs_catch_the_mutation_too(family, mutation):
    cases, fn, _ = FAMILIES[family]
    for case in cases[:4]:
        e, f32 = fn(case, BF16, mutation)
        if mutation == "lse_off":
            assert f32["lse"] > co.LSE_TOL, (case, f32)
        else:
            assert f32["cnt"] > 0, case              # row_cnt differs from the reference count


# ------------------------------------------------------------------------------------------------------------------ the table reaches every path
def test_two_kernel_table_reaches_every_path():
    shapes = {(c.V, c.ld) for c in co.CE_TWO_CASES}
    assert shapes == set(co.TWO_SHAPES)
    for dtype in co.DTYPES3:
        N = co.NVEC[dtype]
        trip = 256 * N
        assert any(V < N for V, _ in shapes), "a case with no full vector"
        assert any(V % N and V > N for V, _ in shapes), "a scalar tail behind full vectors"
        assert any(V % N == 0 for V, _ in shapes), "no scalar tail"
        assert any(V // N > 256 for V, _ in shapes), "a second trip of the forward's 256-thread vector loop"
        assert any(ld // N > 256 and V // N <= 256 for V, ld in shapes) or N == 4, "a second trip of the backward's loop alone"
        assert any(ld // N - (V + N - 1) // N >= 2 for V, ld in shapes), "two whole padding vectors"
        if N == 8:
            assert (trip, trip) in shapes, "exactly one trip"
        for case in co.CE_TWO_CASES:
            R, ignored, per, t = co.ce_layout(case, dtype)
            assert R <= co.MAX_ROWS and t[ignored] == co.IGNORE and sum(x == co.IGNORE for x in t) == 1
            flat = {c for r in range(R) if r != ignored for c in per[r]}
            want = {c for c in (0, case.V - 1, case.V // N * N - 1, case.V // N * N, 2047, 2048) if 0 <= c < case.V and c != co.IGNORE}
            assert flat == want and want <= set(t), "every seam column is planted and carries a target"
            assert all(t[r] in per[r] for r in range(R) if r != ignored)
    assert {c.g for c in co.CE_TWO_CASES} == {1.0, 0.37, 128.0} and {c.regime for c in co.CE_TWO_CASES} == set(co.REGIMES)


def test_fused_table_reaches_every_path():
    cases = co.CE_FUSED_CASES
    assert {co.nv_of(c.ld) for c in cases} == {1, 2, 4, 7, 8}
    assert {c.ld for c in cases} >= set(co.FUSED_LD)
    for lo, hi in ((8192, 8200), (16384, 16392), (32768, 32776), (57344, 57352)):           # both sides of every NV boundary
        assert co.nv_of(lo) < co.nv_of(hi)
    assert co.nv_of(65536) == 8
    for ld in co.FUSED_LD:
        Vs = {c.V for c in cases if c.ld == ld}
        assert Vs >= {v for v in (ld, ld - 3, ld - 11) if v > 0}, ld
        for nv in (co.nv_of(ld),):
            assert {c.g for c in cases if co.nv_of(c.ld) == nv} >= {1.0, 0.37, 128.0}
    assert any(c.V % 8 and c.V > 8 for c in cases) and any(c.V < 8 for c in cases)
    assert any(c.ld // 8 - (c.V + 7) // 8 >= 1 and c.V % 8 for c in cases), "a whole padding vector behind a partial one"
    assert any(c.ld == co.WIDE[1] and c.ld - c.V > 64 for c in cases), "a view of wider storage"
    ends = set()
    for case in cases:
        R, ignored, per, t = co.ce_layout(case, BF16)
        assert R <= co.MAX_ROWS and sum(x == co.IGNORE for x in t) == 1
        flat = {c for r in range(R) if r != ignored for c in per[r]}
        for k in range(1, (case.V + 8191) // 8192):                                          # each side of each slab seam inside the row
            assert 8192 * k - 1 in flat and (8192 * k in flat or 8192 * k >= case.V), (case, k)
        assert {0, case.V - 1} <= flat
        if case.V >= 8:
            assert case.V // 8 * 8 - 1 in flat and (case.V // 8 * 8 in flat or case.V % 8 == 0)
        if case.V > 1536:
            assert {1535, 1536} <= flat                                                      # a wave seam inside a slab
        assert all(t[r] in per[r] for r in range(R) if r != ignored)
        own = {c for c in (0, case.V - 1, case.V // 8 * 8 - 1, case.V // 8 * 8) if 0 <= c < case.V and c != co.IGNORE}
        if own <= set(t):
            ends.add((case.V, case.ld))
    assert ends == {(c.V, c.ld) for c in cases}, "for every (V, ld) one case has targets on the row ends and the last full vector's edge"
    for ld in co.FUSED_LD + (co.WIDE[1],):                      # targets: between the cases of one ld EVERY seam column carries one
        targets, seams = set(), set()
        for case in cases:
            if case.ld == ld:
                R, ignored, per, t = co.ce_layout(case, BF16)
                targets |= {t[r] for r in range(R) if r != ignored}
                seams |= {c for r in range(R) if r != ignored for c in per[r]}
        assert seams <= targets, (ld, sorted(seams - targets))
        Vm = max(c.V for c in cases if c.ld == ld and c.V < ld)                       # (ld - 3; the view of wider storage: its V)
        for k in range(1, (Vm + 8191) // 8192):
            assert {8192 * k - 1, 8192 * k} <= targets, (ld, k)
        if Vm > 1536:
            assert {1535, 1536} <= targets, ld
    assert len({c.seed for c in cases}) == len(cases)


def test_label_smoothing_and_probs_tables_are_the_ones_asked_for():
    ls = co.LS_CASES
    assert {c.V for c in ls} == set(co.LS_V) and {c.eps for c in ls} == {0.0, 0.1} and any(c.pad == 24 for c in ls)
    for V in co.LS_V:
        have = {(c.variant, c.crange, c.eps) for c in ls if c.V == V and c.pad == 0}
        for eps in (0.0, 0.1):
            assert ("none", None, eps) in have and ("mask", None, eps) in have
            assert any(v == "both" and e == eps for v, _, e in have)
            for r in ((4, V), (7, V - 2), (255, 257)):
                if r[1] > r[0] and r[1] <= V:
                    assert ("range", r, eps) in have, (V, r)
    assert 0.0 in co.LS_ROW_W and co.LS_ROW_W[co.LS_IGNORED] != 0
    assert {(c.regime, c.eps) for c in ls if c.pad == 0} == {(rg, e) for rg in co.REGIMES for e in (0.0, 0.1)}
    for variant in ("none", "range", "mask", "both"):
        assert {c.regime for c in ls if c.variant == variant} == set(co.REGIMES), variant
    assert co.LS_GRADED == (0, 3, 4, 5)
    edges, foreign_seen = set(), 0
    for c in ls:
        t, own, foreign = co.ls_layout(c)
        seams = co.ls_seams(c)
        assert t[co.LS_IGNORED] == co.IGNORE and sum(x == co.IGNORE for x in t) == 1
        if c.crange is not None:
            assert {c.crange[0], c.crange[1] - 1} <= set(t) and c.crange[1] - 1 in seams, c
            edges.add(c.crange)
        if c.crange is None or c.crange[1] == c.V:
            assert c.V - 1 in seams, c
        if c.V > 256 and (c.crange is None or c.crange[0] <= 255 < 256 < c.crange[1]):
            assert {255, 256} <= set(seams), c
        # every seam column is planted in a row whose gradient is checked, and is allowed there: its bound is positive
        b = co.build_ls(c, BF16)
        _, bd = co.lsce_reference(b["x"], b["t"], b["g"], b["eps"], crange=b["crange"], cmask=b["cmask"], row_w=b["row_w"])
        for col in seams:
            assert any(col in own[r] and float(bd[r, col]) > 0 for r in co.LS_GRADED), (c, col)
        if c.variant in ("mask", "both"):
            m = b["cmask"]
            for col in co.LS_SPECIAL(c.V):
                assert bool(m[:, col].any()) and not bool(m[:, col].all()), (c, col)
            assert all(bool(m[r, t[r]]) for r in range(co.LS_ROWS))
            for r in range(co.LS_ROWS):                          # a dominant logit the mask disallows: its bound is zero
                for col in foreign[r]:
                    assert not bool(m[r, col]) and float(bd[r, col]) == 0.0, (c, r, col)
                    foreign_seen += 1
    assert (255, 257) in edges and foreign_seen >= 8
    pc = co.P_CASES
    assert {(c.V, c.pad, c.log_probs, c.regime) for c in pc} == {(V, pad, lp, rg) for V in co.P_V for pad in (0, 8) for lp in (True, False)
                                                                 for rg in co.REGIMES}
    assert len({c.seed for c in pc}) == len(pc)


# ------------------------------------------------------------------------------------------------------------------ the floor
def _floor_share(d_bound, dtype, g):
    """Share of the live elements whose underflow floor exceeds 1 % of eps * bound, and the mask of those elements."""
    live = d_bound > 0
    hidden = live & (co.floor_of(dtype, g) > 0.01 * co.EPS[dtype] * d_bound)
    return float(hidden.sum()) / max(1, int(live.sum())), hidden


def _bounds_of(family, case, dtype):
    """-> (bound [R, ld], g, [(row, column)] of the planted and target columns that are live)."""
    if family.startswith("ce"):
        b = co.build_ce(case, dtype)
        _, bd = co.ce_reference(b["x"], b["t"], b["g"])
        keys = [(r, int(b["t"][r])) for r in range(len(b["cols"])) if r != b["ignored"]]
        if case.regime == "planted":
            keys += [(r, c) for r in range(len(b["cols"])) if r != b["ignored"] for c in b["cols"][r]]
        return bd, b["g"], keys
    b = co.build_ls(case, dtype)
    _, bd = co.lsce_reference(b["x"], b["t"], b["g"], b["eps"], crange=b["crange"], cmask=b["cmask"], row_w=b["row_w"])
    t, own, _ = co.ls_layout(case)
    keys = [(r, t[r]) for r in range(co.LS_ROWS)] + ([(r, c) for r in range(co.LS_ROWS) for c in own[r]] if case.regime == "planted" else [])
    return bd, b["g"], [(r, c) for r, c in keys if float(bd[r, c]) > 0]


@pytest.mark.parametrize("family", ["ce_two", "ce_fused", "lsce"])
def test_the_floor_hides_nothing_that_matters(family):
    """bf16: no element's floor exceeds 1 % of eps * bound.  fp16 (subnormals end at 2^-24, the small probabilities lie below): the share
    of such elements is printed per case, and the planted and the target columns are never among them.  Every fp16 case is the bf16
    case of the same table entry."""
    cases = FAMILIES[family][0]
    assert BF16 in FAMILIES[family][2] and FP16 in FAMILIES[family][2]          # one table for both: each fp16 case has its bf16 twin
    for case in cases:
        bd, g, _ = _bounds_of(family, case, BF16)
        share, _ = _floor_share(bd, BF16, g)
        assert share == 0.0, (case, share)
    lines = []
    for case in cases:
        bd, g, keys = _bounds_of(family, case, FP16)
        share, hidden = _floor_share(bd, FP16, g)
        lines.append(f"{share:.3f} {tuple(case)}")
        for r, c in keys:
            assert not bool(hidden[r, c]), (case, r, c)
    print(f"\n{family}: fp16 share of live elements with floor > 1 % of eps * bound\n  " + "\n  ".join(lines))


def test_probs_gradients_lie_above_the_floor():
    for case in co.P_CASES:
        for dtype in (BF16, FP16):
            b = co.build_probs(case, dtype)
            y = co.probs_emulate(b["x"], case.log_probs)
            _, bd = co.probs_bwd_reference(b["dy"], y, co.bwd_ld(case.V), case.log_probs)
            share, hidden = _floor_share(bd, dtype, co.PLANT_DY)
            if dtype == BF16:
                assert share == 0.0, case
            for r, cs in enumerate(b["cols"]):
                assert case.regime != "planted" or not bool(hidden[r, cs[0]]), (case, r)
