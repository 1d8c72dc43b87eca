"""CPU: the row-normalisation oracle (tests/rownorm_oracle.py) is sound before a GPU is touched -- the float32 emulation of the kernels'
rounding points stays under CEILING against the float64 reference over every table, regime and dtype (fp32 tensors and the fp32 row
statistics within 1/8 of what the GPU tests allow), every named mutation of the emulation exceeds the kernel tolerance on a case of the
table that claims to cover it, the library's host-only entry points confirm the route every case claims, and the entry points refuse
what they document with the documented codes.  Run with -s for the measured ceilings and the case that catches each mutation."""
import functools

import pytest
import torch

from ofasys_amd import lib as L
from tests import rownorm_oracle as ro

BF16, FP16, F32 = ro.BF16, ro.FP16, ro.F32
CODE = {F32: L.F32, BF16: L.BF16, FP16: L.F16}
OK, INVALID, UNSUPPORTED = 0, 1, 2
BIG = 1 << 18                        # elements: cases above it meet only the mutations that need their row count


def fwd_eval(case, dtype, mutation=None):
    b = ro.build_ln_fwd(case, dtype)
    return ro.ln_fwd_figures(b, ro.ln_emulate(b["x"], b["gamma"], b["beta"], b["eps"], dtype, b["gelu"], mutation), dtype)


def bwd_eval(case, dtype, mutation=None):
    b = ro.build_ln_bwd(case, dtype)
    got = ro.ln_bwd_emulate(b["dy"], b["x"], b["gamma"], b["mean"], b["rstd"], dtype, b["gelu"], b["dres"], b["prev"], b["want_dbias"],
                            mutation)
    return ro.ln_bwd_figures(b, got, dtype)


def join_eval(case, dtype, mutation=None):
    c = ro.build_join(case, dtype)
    return ro.join_figures(c, ro.join_emulate(c, dtype, mutation), dtype)


FAMILIES = {"ln_fwd": (ro.LN_FWD_CASES, fwd_eval), "ln_bwd": (ro.LN_BWD_CASES, bwd_eval), "join": (ro.JOIN_CASES, join_eval)}


def _size(family, case):
    return case.rows * (ro.join_cols(case, BF16) if family == "join" else case.m * 8)


def test_constants_hang_together():
    assert ro.TOL == 2 * ro.CEILING and ro.CEILING <= 1.1
    assert ro.EPS == {BF16: 2.0 ** -8, FP16: 2.0 ** -11}
    assert max(c.rows * c.m * 8 for c in ro.LN_BWD_CASES) <= 513 * 8192 and max(_size("join", c) for c in ro.JOIN_CASES) <= 2049 * 1024
    for cases in (ro.LN_FWD_CASES, ro.LN_BWD_CASES, ro.JOIN_CASES, ro.forced_join_cases()):
        assert len({c.name for c in cases}) == len(cases) and len({c.seed for c in cases}) == len(cases)


@pytest.mark.parametrize("family,dtype", [(f, d) for f in FAMILIES for d in ro.DTYPES3], ids=[f"{f}-{ro.NAMES[d]}" for f in FAMILIES for d in ro.DTYPES3])
def test_emulation_stays_within_the_ceiling(family, dtype):
    """Every output of every case: 16-bit tensors <= CEILING in eps of the magnitude bound; fp32 tensors and the row statistics within
    1/8 of the GPU tolerance."""
    cases, fn = FAMILIES[family]
    worst = {}
    for case in cases:
        for n, v in fn(case, dtype).items():
            if v > worst.get(n, (-1.0, None))[0]:
                worst[n] = (v, case.name)
    print(f"\n{family} {ro.NAMES[dtype]}: " + "; ".join(f"{n} {v:.3g} ({w})" for n, (v, w) in sorted(worst.items())))
    for n, (v, w) in worst.items():
        assert v <= ro.limit(family, n, dtype, kernel=False), (n, v, w)


# ------------------------------------------------------------------------------------------------------------------ mutations
def _applies(family, m, case):
    if family == "ln_fwd":
        return {"padded_mean": case.m % 64 != 0, "tanh_gelu": case.gelu}.get(m, True)
    if family == "ln_bwd":
        r = ro.ln_bwd_route(case.m, case.gelu)
        return {"gamma_no_part_offset": r.wpr > 1, "stale_ring_slot": case.rows > ro.LN_BLOCKS * r.rpb, "no_dres": case.dres,
                "accumulate_overwrites": case.acc, "dbias_before_gelu": case.dbias, "gelu_no_xphi": case.gelu}.get(m, True)
    drop = case.p > 0
    return {"no_scale": drop, "mask_shift": drop, "dropout_before_lna": drop and case.a, "dres_missing_dy": case.b and case.dy,
            "dres_dropped": drop and case.want_dres, "colsum_before_lna": case.a and case.xsum, "ignore_residual": case.res,
            "stats_b_unrounded": case.b}[m]


NEEDS_ROWS = ("stale_ring_slot",)
MUTANTS = [("ln_fwd", m) for m in ro.LN_FWD_MUTATIONS] + [("ln_bwd", m) for m in ro.LN_BWD_MUTATIONS] + [("join", m) for m in ro.JOIN_MUTATIONS]


@functools.lru_cache(maxsize=None)
def _clean(family, case):
    return FAMILIES[family][1](case, BF16)


@pytest.mark.parametrize("family,mutation", MUTANTS, ids=[f"{f}-{m}" for f, m in MUTANTS])
def test_table_and_metric_catch_the_mutation(family, mutation):
    """Each subtly wrong variant of the emulation exceeds what the GPU test allows a kernel (bf16) in at least one case of the table it
    applies to, while the unmutated emulation of that case stays under the ceiling.  A mutation no case catches fails here by name."""
    cases, fn = FAMILIES[family]
    caught, tried = [], 0
    for case in cases:
        if not _applies(family, mutation, case) or (_size(family, case) > BIG and mutation not in NEEDS_ROWS):
            continue
        tried += 1
        over = {n: v for n, v in fn(case, BF16, mutation).items() if v > ro.limit(family, n, BF16, kernel=True)}
        if over:
            for n, v in _clean(family, case).items():
                assert v <= ro.limit(family, n, BF16, kernel=False), (case.name, n, v)
            caught.append((case.name, over))
    assert caught, f"no case of the {family} table notices {mutation} ({tried} tried): the table is missing a case"
    name, over = caught[0]
    print(f"\n{family} {mutation}: caught in {len(caught)} of {tried} cases, first by [{name}] through " +
          ", ".join(f"{n} {v:.3g}" for n, v in sorted(over.items())))


# ------------------------------------------------------------------------------------------------------------------ no blind cases
SEES = 0.25                   # eps: a clean figure below it means the bound dwarfs the value, and a check of it sees nothing


def test_every_route_has_a_case_that_sees():
    """A case whose bound is hundreds of times the values passes whatever the kernel does, and must not count as coverage: for every
    backward instantiation (GELU, WPR, NV) and every join route and flag combination, some case's CLEAN bf16 figure reaches SEES eps
    on every output (dbias on every GELU route), i.e. the output's own rounding is visible against its bound.  (Single cases may
    fall below it by honest cancellation -- a column sum over thousands of rows, the dx of the planted row -- or sit at 0 where the
    join copies dy through; every join case sees on y.)"""
    groups = {}
    for c in ro.LN_BWD_CASES:
        r = ro.ln_bwd_route(c.m, c.gelu)
        fig = _clean("ln_bwd", c)
        g = groups.setdefault(("ln_bwd", c.gelu, r.wpr, r.nv), {})
        for n, v in fig.items():
            g[n] = max(g.get(n, 0.0), v)
    for key, g in groups.items():
        assert set(g) >= {"dx", "dgamma", "dbeta"} | ({"dbias"} if key[1] else set()), key
    for c in ro.JOIN_CASES:
        r = ro.join_route(ro.join_cols(c, BF16), BF16, True, c.keep)
        fig = _clean("join", c)
        g = groups.setdefault(("join", r.kind, r.k or r.wpr, c.a, c.b, c.p > 0), {})
        for n, v in fig.items():
            if n == "dx_colsum":                     # (asked for in a few cases only: per kernel and shape, not per flag combination)
                k = groups.setdefault(("join", r.kind, r.k or r.wpr), {})
                k[n] = max(k.get(n, 0.0), v)
            elif not n.startswith(("mean", "rstd")) and n != "ydrop":
                g[n] = max(g.get(n, 0.0), v)
        assert fig["y"] >= SEES, (c.name, fig)
    for key, g in groups.items():
        blind = {n: v for n, v in g.items() if v < SEES and not (key[0] == "join" and n in ("dx", "dres") and v == 0.0)}
        assert not blind, (key, blind)
    print(f"\n{len(groups)} routes, each with a seeing case for every output")


# ------------------------------------------------------------------------------------------------------------------ the routes are real
def test_tables_claim_every_route_the_dispatchers_can_launch():
    """By plain arithmetic on the restated dispatch: the forward table reaches every NV on both sides of its boundary; the backward
    table every (NV, WPR, GELU) instantiation that any accepted row width reaches; the join table every row-per-wave k in both
    directions, every flag instantiation of the row-per-wave backward, every split-row WPR (full and ragged) and forward NV."""
    assert {ro.ln_fwd_nv(c.m) for c in ro.LN_FWD_CASES} == {1, 2, 4, 8, 16, 32} and ro.ln_fwd_nv(ro.FWD_REFUSED_M) is None
    for lo in (64, 128, 256, 512, 1024):
        assert {lo, lo + 1} <= set(ro.FWD_M) and ro.ln_fwd_nv(lo) < ro.ln_fwd_nv(lo + 1)
    assert {(c.rows, c.gelu) for c in ro.LN_FWD_CASES} == {(r, g) for r in (1, 3, 5) for g in (False, True)}
    for gelu in (False, True):
        reachable = {(r.wpr, r.nv, r.pf) for r in (ro.ln_bwd_route(m, gelu) for m in range(1, 4097)) if r is not None}
        claimed = {(r.wpr, r.nv, r.pf) for r in (ro.ln_bwd_route(c.m, c.gelu) for c in ro.LN_BWD_CASES if c.gelu == gelu)}
        assert claimed == reachable, (gelu, sorted(reachable - claimed))
        assert (6, 1, 2) in claimed if gelu else all(pf == 0 and (w == 1 or nv > 1) for w, nv, pf in claimed)
    assert ro.ln_bwd_route(ro.BWD_REFUSED_M, False) is None and ro.ln_bwd_route(ro.BWD_REFUSED_M, True) is None
    for gelu, m in ro.ROW_SWEEP:                                  # per WPR: 1, rpb - 1, rpb + 1 rows and one live row in the second sweep
        r = ro.ln_bwd_route(m, gelu)
        rows = {c.rows for c in ro.LN_BWD_CASES if (c.gelu, c.m) == (gelu, m)}
        assert rows >= {1, r.rpb + 1, ro.LN_BLOCKS * r.rpb + 1} | ({r.rpb - 1} - {0}), (gelu, m, rows)
        seams = {(c.rows, c.seam_row) for c in ro.LN_BWD_CASES if (c.gelu, c.m, c.regime) == (gelu, m, "prow")}
        assert {(r.rpb + 1, r.rpb - 1), (r.rpb + 1, r.rpb), (ro.LN_BLOCKS * r.rpb + 1, ro.LN_BLOCKS * r.rpb)} <= seams
        if r.pf:
            assert 2 * ro.LN_BLOCKS * r.rpb + 1 in rows                                   # niter 1, 2 and 3 through the ring
    assert {ro.ln_bwd_route(m, g).wpr for g, m in ro.ROW_SWEEP} == {1, 2, 4, 6, 8}
    assert {(c.gelu, c.dbias) for c in ro.LN_BWD_CASES if c.gelu} == {(True, False), (True, True)}
    # the join
    for dt in (BF16, FP16):
        fwd = {ro.join_route(ro.join_cols(c, dt), dt, False) for c in ro.JOIN_CASES}
        assert {r.k for r in fwd if r.kind == "row"} == {1, 2, 3, 4, 5, 6} and {r.nv for r in fwd if r.kind == "split"} == {1, 2, 4, 8}
        row = {(ro.join_route(ro.join_cols(c, dt), dt, True, c.keep).k, c.a, c.b, c.p > 0) for c in ro.JOIN_CASES
               if ro.join_route(ro.join_cols(c, dt), dt, True, c.keep).kind == "row"}
        assert row == {(k, a, b, d) for k in (1, 2, 3, 4) for a in (False, True) for b in (False, True) for d in (False, True)}
        split = [(c, ro.join_route(ro.join_cols(c, dt), dt, True, c.keep)) for c in ro.JOIN_CASES]
        split = [(c, r) for c, r in split if r.kind == "split"]
        assert {r.wpr for _, r in split} == {1, 2, 4, 8}
        assert {r.wpr for c, r in split if (ro.join_cols(c, dt) // 8 // r.wpr) % 64} == {1, 2, 4, 8}, "a ragged part for every WPR"
        assert any(c.cols and not c.keep and c.p > 0 for c, _ in split), "a 256 k shape whose backward regenerates the mask"
        assert {c.cols for c, _ in split if c.cols} >= {1280, 1536}
    assert {ro.join_route(ro.join_cols(c, F32), F32, True).kind for c in ro.JOIN_CASES} == {"split"}
    assert {ro.join_route(ro.join_cols(c, F32), F32, True).wpr for c in ro.JOIN_CASES} == {1, 2, 4, 8}
    flags = ro.JOIN_CASES
    assert any(not c.dy for c in flags) and any(not c.res for c in flags) and any(not c.want_dres for c in flags)
    assert any(c.xsum for c in flags) and any(c.base for c in flags)
    assert {c.rows for c in flags} >= {1, 7, 2049, 4097} and all(ro.join_cols(c, BF16) <= 1024 for c in flags if c.rows > 2048)
    for dt, cols in ro.JOIN_REFUSED:
        assert ro.join_route(cols, dt, False) is None and ro.join_route(cols, dt, True) is None, (dt, cols)
    forced = ro.forced_join_cases()
    assert {(c.cols // 256, c.a, c.b, c.p > 0) for c in forced} == {(k,) + f for k in (1, 2, 3, 4) for f in
                                                                    ((a, b, d) for a in (False, True) for b in (False, True) for d in (False, True))}
    assert {c.rows for c in forced} == {1, 7, 2049} and all({c.rows for c in forced if c.cols == 256 * k} == {1, 7, 2049} for k in (1, 2, 3, 4))


def test_library_confirms_the_route_of_every_case():
    """ofa_layernorm_bwd_slots at a probing row count reveals the rows per block iteration of the route a case claims (16 / WPR; 2 for
    the 12-wave six-waves-per-row blocks as for WPR 8); ofa_join_bwd_slots the same for the join; ofa_join_keep_bytes is non-zero exactly
    where the backward is the row-per-wave kernel.  A dispatch change that moves a case off its route fails here."""
    h = L.lib().cdll
    probe = 48                                                     # ceil(48 / rpb) is distinct for rpb = 16, 12, 8, 6, 4, 3, 2
    for dt in ro.DTYPES3:
        N = ro.NVEC[dt]
        for c in ro.LN_BWD_CASES:
            r = ro.ln_bwd_route(c.m, c.gelu)
            assert h.ofa_layernorm_bwd_slots(probe, c.m * N, CODE[dt], int(c.gelu)) == ro.cdiv(probe, r.rpb), c.name
            assert h.ofa_layernorm_bwd_slots(c.rows, c.m * N, CODE[dt], int(c.gelu)) == min(ro.LN_BLOCKS, ro.cdiv(c.rows, r.rpb)), c.name
        for c in ro.JOIN_CASES + ro.forced_join_cases():
            cols = ro.join_cols(c, dt)
            r = ro.join_route(cols, dt, True)
            assert h.ofa_join_bwd_slots(probe, cols, CODE[dt]) == ro.cdiv(probe, r.rpb), (c.name, ro.NAMES[dt])
            assert h.ofa_join_keep_bytes(c.rows, cols, CODE[dt]) == ro.join_keep_bytes(c.rows, cols, dt), (c.name, ro.NAMES[dt])
            assert (h.ofa_join_keep_bytes(c.rows, cols, CODE[dt]) > 0) == (r.kind == "row")


# ------------------------------------------------------------------------------------------------------------------ refusals
_P = 4096                     # a fake, 16-byte aligned device address: every call below is refused before any launch


def _ln_fwd(h, name, cols, dt, rows=4, x=_P, g=_P, b=_P, y=_P):
    return getattr(h, name)(x, g, b, y, None, None, rows, cols, 1e-5, dt, None)


def _ln_bwd(h, name, cols, dt, rows=4, **null):
    a = dict(dy=_P, x=_P, gamma=_P, mean=_P, rstd=_P, dx=_P, dgamma=_P, dbeta=_P, ws=_P)
    a.update(null)
    if name == "ofa_layernorm_bwd":
        return h.ofa_layernorm_bwd(a["dy"], a["x"], a["gamma"], a["mean"], a["rstd"], None, a["dx"], a["dgamma"], a["dbeta"], a["ws"], rows, cols,
                                   0, dt, None)
    return h.ofa_gelu_layernorm_bwd(a["dy"], a["x"], a["gamma"], a["mean"], a["rstd"], a["dx"], a["dgamma"], a["dbeta"], None, a["ws"], rows,
                                    cols, 0, dt, None)


def test_layernorm_entry_points_refuse_with_their_documented_codes():
    """Null pointers: OFA_ERR_INVALID; a row width that is no multiple of the vector, wider than 32 slabs (forward) or than 8 vectors
    per lane after the split (backward: 4104 columns in 16 bits): OFA_ERR_UNSUPPORTED -- shapes the forward accepts included."""
    h = L.lib().cdll
    for dt in ro.DTYPES3:
        N, code = ro.NVEC[dt], CODE[dt]
        for name in ("ofa_layernorm_fwd", "ofa_gelu_layernorm_fwd"):
            assert _ln_fwd(h, name, 2048 * N, code, rows=0) == OK                                   # the widest row is accepted
            assert _ln_fwd(h, name, ro.FWD_REFUSED_M * N, code) == UNSUPPORTED                       # 16384 + 8 columns
            assert _ln_fwd(h, name, N + 1, code) == UNSUPPORTED and _ln_fwd(h, name, 0, code) == INVALID
            assert _ln_fwd(h, name, 8 * N, code, rows=-1) == INVALID and _ln_fwd(h, name, 8 * N, 7) == INVALID
            for null in ("x", "g", "b", "y"):
                assert _ln_fwd(h, name, 8 * N, code, **{null: None}) == INVALID, (name, null)
        for name in ("ofa_layernorm_bwd", "ofa_gelu_layernorm_bwd"):
            assert _ln_bwd(h, name, ro.BWD_REFUSED_M * N, code) == UNSUPPORTED                       # the forward takes this width
            assert _ln_fwd(h, "ofa_layernorm_fwd", ro.BWD_REFUSED_M * N, code, rows=0) == OK
            assert _ln_bwd(h, name, 4097 * N, code) == UNSUPPORTED and _ln_bwd(h, name, N + 1, code) == UNSUPPORTED
            assert _ln_bwd(h, name, 8 * N, 7) == INVALID and _ln_bwd(h, name, 8 * N, code, rows=-1) == INVALID
            for null in ("dy", "x", "gamma", "mean", "rstd", "dx", "dgamma", "dbeta", "ws"):
                assert _ln_bwd(h, name, 8 * N, code, **{null: None}) == INVALID, (name, null)
            for m in ro.PLAIN_M + ro.GELU_M:                                                         # accepted: refused only for the null
                assert _ln_bwd(h, name, m * N, code, ws=None) == INVALID, (name, m)


def _join_fwd(h, cols, dt, rows=4, x=_P, y=_P, stats=_P, ga=_P, ba=_P, gb=_P, bb=_P, z=_P, p=0.1):
    return h.ofa_join_fwd(x, _P, ga, ba, gb, bb, y, z, stats, None, rows, cols, 1e-5, p, 1, 0, None, dt, None)


def _join_bwd(h, cols, dt, rows=4, dy=_P, dz=_P, x=_P, y=_P, ga=_P, gb=_P, stats=_P, dx=_P, ws=_P):
    return h.ofa_join_bwd(dy, dz, x, y, ga, gb, stats, None, _P, dx, ws, rows, cols, 0.1, 1, 0, None, 0, dt, None)


def test_join_entry_points_refuse_with_their_documented_codes():
    """Columns that do not split over the waves (1032 in bf16: 129 vectors over 4 waves; 520, 1800) or exceed 8 x 64 vectors:
    OFA_ERR_UNSUPPORTED from both directions; missing tensors, half a LayerNorm, p outside [0, 1): OFA_ERR_INVALID."""
    h = L.lib().cdll
    for dt, cols in ro.JOIN_REFUSED:
        assert _join_fwd(h, cols, CODE[dt]) == UNSUPPORTED and _join_bwd(h, cols, CODE[dt]) == UNSUPPORTED, (dt, cols)
    for dt in ro.DTYPES3:
        code = CODE[dt]
        for c in ro.JOIN_CASES:                                     # every shape of the table is accepted: refused only for the null
            assert _join_fwd(h, ro.join_cols(c, dt), code, rows=0) == OK and _join_bwd(h, ro.join_cols(c, dt), code, rows=0) == OK, c.name
            assert _join_fwd(h, ro.join_cols(c, dt), code, x=None) == INVALID and _join_bwd(h, ro.join_cols(c, dt), code, dx=None) == INVALID
        for null in ("x", "y", "stats", "ba", "ga", "bb", "z"):
            assert _join_fwd(h, 256, code, **{null: None}) == INVALID, null
        assert _join_fwd(h, 256, code, p=1.0) == INVALID and _join_fwd(h, 256, code, p=-0.5) == INVALID
        assert _join_fwd(h, 256, 7) == INVALID and _join_bwd(h, 256, 7) == INVALID
        for null in ("stats", "dx", "ws", "x", "y", "dz"):
            assert _join_bwd(h, 256, code, **{null: None}) == INVALID, null
        assert _join_bwd(h, 256, code, dy=None, dz=None, gb=None) == INVALID
        assert _join_fwd(h, 256, code, rows=-1) == UNSUPPORTED and _join_bwd(h, 256, code, rows=-1) == UNSUPPORTED
