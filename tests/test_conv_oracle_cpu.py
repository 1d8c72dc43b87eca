"""CPU: the convolution-stack oracle (tests/conv_oracle.py) is sound before a GPU is touched -- every case claims the route the restated
dispatch and the library's host-only entry points (ofa_batchnorm_route, ofa_im2col_route) give it; over the BatchNorm table a row lane of
the statistics kernel executes 0, 1, 2, 3 and >= 5 rows; the float32 emulation stays under CEILING against the float64 reference (fp32
tensors and the statistics within 1/8 of what the GPU test allows); every named mutation is rejected by a named case; no element of a
recomputed-gate case is gate-ambiguous, under the float64 statistics and under statistics perturbed by their tolerances; the exact
families are exact (integer sums below 256, the pool oracle equals torch's).  Run with -s for the measured figures."""
import functools

import pytest
import torch
import torch.nn.functional as F

from ofasys_amd import lib as L
from tests import conv_oracle as co

BF16, FP16, F32 = co.BF16, co.FP16, co.F32
CODE = {F32: L.F32, BF16: L.BF16, FP16: L.F16}
IDS = [co.NAMES[d] for d in co.DTYPES3]
OK, INVALID, UNSUPPORTED = 0, 1, 2


def _size(case, dtype=BF16):
    return (case.rows + case.nb) * co.bn_cols(case, dtype)


def test_constants_hang_together():
    assert co.TOL == 2 * co.CEILING and co.CEILING <= 1.1 and co.GATE_MARGIN == 2.0 ** -12
    for cases in (co.BN_CASES, co.IM2COL_CASES, co.COL2IM_CASES, co.MAXPOOL_CASES):
        assert len({c.name for c in cases}) == len(cases) and len({c.seed for c in cases}) == len(cases)
    assert sum(_size(c) > co.BIG for c in co.BN_CASES) == 3 and max(_size(c) for c in co.BN_CASES) <= 32897 * 256
    assert len(set(co.FLAGS)) == len(co.FLAGS) and all(g != "x" or (r and not s and not d) for _, r, s, g, d in co.FLAGS)


# ------------------------------------------------------------------------------------------------------------------ routes
def test_batchnorm_table_reaches_every_seam():
    """Plain arithmetic on the restated dispatch: cw takes 1, 2, 8, 16 and 32, one column block holds a single vector (m = 33, 129),
    C % 16 != 0 occurs; over the table a row lane of the statistics kernel executes 0 rows, exactly 1 (tail only), 2 (pair only),
    3 (pair + tail) and >= 5; rows = 1; the group cap exactly and binding; the second sweep of the apply / dx kernels; the second trip of
    bn_fold_groups; the second block of bn_eval_stats_kernel; both gate routes and none, in training and in eval mode."""
    bn = [c for c in co.BN_CASES if c.m]
    assert {1 << co.bn_cw_log2(c.m) for c in bn} == {1, 2, 8, 16, 32}
    assert any(c.m % 32 == 1 for c in bn) and any(co.bn_cols(c, BF16) % 16 for c in co.BN_CASES)
    seen = set()
    for c in co.BN_CASES:
        for dt in co.DTYPES3:
            rows, m = c.rows, co.bn_m(c, dt)
            step = co.bn_step(rows, m)
            counts = {len(range(lane, rows, step)) for lane in range(step)}
            assert counts == co.lane_rows(rows, m) | ({0} if rows < step else set()), c.name
            seen |= counts
            keep = co.kept_rows(rows, m)
            assert int((~keep).sum()) == sum(len(range(lane, rows, step)) % 2 for lane in range(step)), c.name
    assert {0, 1, 2, 3} <= seen and max(seen) >= 5, seen
    per_cw = {}
    for c in bn:
        per_cw.setdefault(co.bn_cw_log2(c.m), set()).update(co.lane_rows(c.rows, c.m))
    assert all({2, 3} <= v for k, v in per_cw.items() if k >= 3), per_cw        # (cw 1 and 2: a lane has two rows only above 32768)
    assert any(c.rows == 1 for c in co.BN_CASES)
    assert {(c.rows, co.bn_groups(c.rows)) for c in co.BN_CASES if c.rows >= 32768} == {(32768, 256), (32768 + 129, 256)}
    assert co.bn_groups(32768 - 128) == 255 and cdiv(32768 + 129, 128) > 256
    sweep = [c for c in co.BN_CASES if all(c.rows * co.bn_m(c, dt) > co.SWEEP for dt in co.DTYPES3)]
    assert sweep and any(c.rows == 4100 and c.m == 256 for c in sweep)
    assert {c.G for c in co.BN_CASES if c.mode == "groups"} == {1, 15, 16, 17, 255, 256, 257, 513}
    assert {c.C for c in co.BN_CASES if c.mode == "groups"} == {8, 24, 40}
    assert any(not c.train and co.bn_cols(c, dt) > 256 for c in co.BN_CASES for dt in co.DTYPES3)
    assert all(any(not c.train and co.bn_cols(c, dt) > 256 for c in co.BN_CASES) for dt in co.DTYPES3)
    assert {(c.train, c.gate) for c in co.BN_CASES if c.bwd} == {(t, g) for t in (False, True) for g in ("", "x", "y")}
    assert {c.mom for c in co.BN_CASES} == {0.1, 0.01} and {c.eps for c in co.BN_CASES} == {1e-5, 1e-3}
    assert any(c.acc for c in co.BN_CASES) and any(c.want_dres for c in co.BN_CASES) and {c.regime for c in co.BN_CASES} == set(co.REGIMES)
    sync = [c for c in co.BN_CASES if c.mode == "sync"]
    assert sync and all(c.nb and c.nb != c.rows for c in sync) and {c.gate for c in sync} == {"", "x"}
    assert sum(c.nan for c in co.BN_CASES) == 2 and {c.train for c in co.BN_CASES if c.nan} == {False, True}


def cdiv(a, b):
    return -(-a // b)


def test_library_confirms_the_route_of_every_case():
    """ofa_batchnorm_route and ofa_im2col_route -- which the launchers themselves call -- against the restated dispatch for every entry
    of every table: a dispatch change that moves a case off the route it claims fails here."""
    import ctypes
    h = L.lib().cdll
    out = (ctypes.c_int * 3)()
    for dt in co.DTYPES3:
        for c in co.BN_CASES:
            C = co.bn_cols(c, dt)
            assert h.ofa_batchnorm_route(c.rows, C, CODE[dt], ctypes.addressof(out)) == OK, c.name
            assert tuple(out) == co.bn_route(c.rows, co.bn_m(c, dt)), (c.name, tuple(out))
        assert h.ofa_batchnorm_route(5, co.NVEC[dt] + 1, CODE[dt], ctypes.addressof(out)) == UNSUPPORTED
        assert h.ofa_batchnorm_route(0, 8, CODE[dt], ctypes.addressof(out)) == INVALID and h.ofa_batchnorm_route(5, 8, CODE[dt], None) == INVALID
        for c in co.for_dtype(co.IM2COL_CASES, dt):
            g = co.case_geom(c, dt)
            Ho, Wo = co.geom_out(g)
            assert Ho > 0 and Wo > 0, c.name
            want = co.im2col_route(co.kpad(g), g.C, c.nchw, dt)
            assert want == c.route, (c.name, co.NAMES[dt], want)
            assert h.ofa_im2col_route(g.B, Ho, Wo, g.C, co.kpad(g), int(c.nchw), CODE[dt]) == want, (c.name, co.NAMES[dt])
            assert h.ofa_conv_out_size(g.H, g.kh, g.s, g.p) == Ho and h.ofa_conv_out_size(g.W, g.kw, g.s, g.p) == Wo
        assert {c.route for c in co.for_dtype(co.IM2COL_CASES, dt)} == {0, 1, 2}
        assert {(c.route, c.nchw) for c in co.for_dtype(co.IM2COL_CASES, dt)} == {(0, False), (0, True), (1, False), (2, True)}
        assert {co.case_geom(c, dt).B * co.geom_out(co.case_geom(c, dt))[0] * co.geom_out(co.case_geom(c, dt))[1]
                for c in co.IM2COL_CASES if c.name.startswith("im2col lds stem")} == {6, 64, 65, 390}
        for cases in (co.COL2IM_CASES, co.MAXPOOL_CASES):
            for c in cases:
                g = co.case_geom(c, dt)
                assert min(co.geom_out(g)) > 0 and h.ofa_conv_out_size(g.H, g.kh, g.s, g.p) == co.geom_out(g)[0], c.name
            assert any(max(co.uncovered(co.case_geom(c, dt))) > 0 for c in cases)
            assert sum(g.B * g.H * g.W * (g.C // co.NVEC[dt]) > co.SWEEP for g in (co.case_geom(c, dt) for c in cases)) == 1
        assert h.ofa_im2col_route(1, 1, 1, 8, 8, 0, 7) == -1 and h.ofa_im2col_route(0, 1, 1, 8, 8, 0, CODE[dt]) == -1
    assert h.ofa_conv_out_size(1, 2, 2, 0) == 0 and h.ofa_conv_out_size(1, 3, 3, 0) == 0 and h.ofa_conv_out_size(2, 2, 2, 0) == 1
    assert co.grid_1d(co.SWEEP) == 4096 == co.grid_1d(co.SWEEP + 1) and co.grid_1d(0) == 1
    assert co.RELU_N[-1] > co.SWEEP


# ------------------------------------------------------------------------------------------------------------------ BatchNorm
@functools.lru_cache(maxsize=None)
def _figures(case, dtype, mutation=None):
    c = co.build_bn(case, dtype)
    got = co.bn_emulate(c, dtype, mutation)
    fig = co.bn_figures(c, got, dtype)
    if mutation is None and case.gate == "x" and case.bwd:               # the fp32 evaluation error of the recomputed gate's expression
        mu, var, _ = co._stats64(c)
        t, bd = co.gate_terms(c, mu, 1 / torch.sqrt(var + co._f32(c["eps"])))
        fig["_gate_err"] = float(((got["t32"].double() - t).abs() / bd).max())
    return fig


@pytest.mark.parametrize("dtype", co.DTYPES3, ids=IDS)
def test_emulation_stays_within_the_ceiling(dtype):
    """Every output of every case: 16-bit tensors <= CEILING in eps of the magnitude bound; fp32 tensors and the statistics within 1/8 of
    the GPU tolerance; the fp32 gate expression within 1/100 of GATE_MARGIN."""
    worst = {}
    for case in co.BN_CASES:
        for n, v in _figures(case, dtype).items():
            if v > worst.get(n, (-1.0, None))[0]:
                worst[n] = (v, case.name)
    print(f"\nbatchnorm {co.NAMES[dtype]}: " + "; ".join(f"{n} {v:.3g} ({w})" for n, (v, w) in sorted(worst.items())))
    for n, (v, w) in worst.items():
        if n == "_gate_err":
            assert v * 100 < co.GATE_MARGIN, (v, w)
        else:
            assert v <= co.limit(n, dtype, kernel=False), (n, v, w)


MUT_DTYPE = {"gate_from_unrounded": FP16}                 # a positive value that the stored y holds as 0 exists in fp16 only


@pytest.mark.parametrize("mutation", co.MUTATIONS)
def test_table_and_metric_catch_the_mutation(mutation):
    """Each subtly wrong variant of the emulation exceeds what the GPU test allows a kernel in at least one case of the table, while
    the unmutated emulation of that case stays under the ceiling.  A mutation no case catches fails here by name."""
    dtype = MUT_DTYPE.get(mutation, BF16)
    caught, tried = [], 0
    for case in co.BN_CASES:
        if not co.applies(mutation, case) or _size(case) > co.BIG:
            continue
        tried += 1
        over = {n: v for n, v in _figures(case, dtype, mutation).items() if not n.startswith("_") and v > co.limit(n, dtype, kernel=True)}
        if over:
            for n, v in _figures(case, dtype).items():
                assert n.startswith("_") or v <= co.limit(n, dtype, kernel=False), (case.name, n, v)
            caught.append((case.name, over))
    assert caught, f"no case of the table notices {mutation} ({tried} tried): the table is missing a case"
    name, over = caught[0]
    print(f"\n{mutation}: caught in {len(caught)} of {tried} cases, first by [{name}] through " + ", ".join(f"{n} {v:.3g}" for n, v in sorted(over.items())))


@pytest.mark.parametrize("dtype", co.DTYPES3, ids=IDS)
def test_no_element_is_gate_ambiguous(dtype):
    """Zero elements with |t| < 2^-12 bound under the float64 statistics, and none below half that margin (nor of another sign) when the
    mean moves by the mean tolerance (in units of mean|x|) and rstd by the rstd tolerance, in every combination of signs."""
    n = 0
    for case in co.BN_CASES:
        if not (case.gate == "x" and case.bwd):
            continue
        c = co.build_bn(case, dtype)
        assert int(co.ambiguous(c).sum()) == 0, case.name
        mu, var, am = co._stats64(c)
        rs = 1 / torch.sqrt(var + co._f32(c["eps"]))
        sign = co.gate_terms(c, mu, rs)[0] > 0
        for dm in ((-1, 1) if c["train"] else (0,)):
            for dr in ((-1, 1) if c["train"] else (0,)):
                m2, r2 = mu + dm * co.S32["mean"] * am, rs * (1 + dr * co.S32["rstd"])
                assert int(co.ambiguous(c, m2, r2, co.GATE_MARGIN / 2).sum()) == 0, (case.name, dm, dr)
                assert bool(torch.equal(co.gate_terms(c, m2, r2)[0] > 0, sign)), (case.name, dm, dr)
        n += 1
    assert n >= 8


# ------------------------------------------------------------------------------------------------------------------ exact families
@pytest.mark.parametrize("dtype", co.DTYPES3, ids=IDS)
def test_exact_families_are_exact(dtype):
    """im2col: the reference equals F.unfold on values (NaN-free inputs, taps reordered), pad columns are +0 and the bit patterns
    survive; col2im: the adjoint of im2col, integer sums below 256; the pool oracle equals F.max_pool2d with indices on the NaN-free
    cases, and its backward the scatter of those indices; relu_reference equals torch.relu in value, NaN for NaN."""
    for c in co.for_dtype(co.IM2COL_CASES, dtype):
        g = co.case_geom(c, dtype)
        gen = co._gen(c.seed)
        shape = (g.B, g.C, g.H, g.W) if c.nchw else (g.B * g.H * g.W, g.C)
        x = co.random_bits(shape, dtype, gen)
        assert bool(torch.isfinite(x.float()).all())
        col = co.im2col_reference(x, g, c.nchw)
        K = g.kh * g.kw * g.C
        assert bool((col[:, K:].view(co.INT_VIEW[dtype]) == 0).all())
        img = co._nhwc(x, g, c.nchw).permute(0, 3, 1, 2).double()
        unf = F.unfold(img, (g.kh, g.kw), padding=g.p, stride=g.s)                     # [B, C kh kw, L] in (c, kh, kw) order
        unf = unf.view(g.B, g.C, g.kh * g.kw, -1).permute(0, 3, 2, 1).reshape(-1, K)
        assert bool(torch.equal(col[:, :K].double(), unf)), c.name
    for c in co.COL2IM_CASES:
        g = co.case_geom(c, dtype)
        if g.B * g.H * g.W * g.C > co.BIG and dtype != BF16:
            continue
        Ho, Wo = co.geom_out(g)
        dcol = co.small_ints((g.B * Ho * Wo, co.kpad(g)), dtype, co._gen(c.seed))
        dx = co.col2im_reference(dcol, g)
        assert float(dx.double().abs().max()) < 256 and g.kh * g.kw <= 49
        K = g.kh * g.kw * g.C
        fold = F.fold(dcol[:, :K].double().view(g.B, Ho * Wo, g.kh * g.kw, g.C).permute(0, 3, 2, 1).reshape(g.B, K, Ho * Wo), (g.H, g.W),
                      (g.kh, g.kw), padding=g.p, stride=g.s)
        assert bool(torch.equal(dx.double().view(g.B, g.H, g.W, g.C), fold.permute(0, 2, 3, 1))), c.name
        uh, uw = co.uncovered(g)
        v = dx.view(g.B, g.H, g.W, g.C)
        assert (uh == 0 or bool((v[:, g.H - uh:] == 0).all())) and (uw == 0 or bool((v[:, :, g.W - uw:] == 0).all()))
    for c in co.MAXPOOL_CASES:
        g = co.case_geom(c, dtype)
        if g.B * g.H * g.W * g.C > co.BIG and dtype != BF16:
            continue
        x = co.pool_input(c, g, dtype, co._gen(c.seed))
        y, arg = co.maxpool_reference(x, g)
        Ho, Wo = co.geom_out(g)
        if c.fill != "nan":
            ty, ti = F.max_pool2d(x.float().view(g.B, g.H, g.W, g.C).permute(0, 3, 1, 2), g.kh, g.s, g.p, return_indices=True)
            assert bool(torch.equal(y.float().view(g.B, Ho, Wo, g.C).permute(0, 3, 1, 2), ty)), c.name
            a = arg.view(g.B, Ho, Wo, g.C).permute(0, 3, 1, 2).long()
            oh, ow = torch.arange(Ho).view(1, 1, -1, 1), torch.arange(Wo).view(1, 1, 1, -1)
            flat = (oh * g.s - g.p + a // g.kw) * g.W + (ow * g.s - g.p + a % g.kw)
            live = ty > float("-inf")                                                    # (a window of nothing but -inf: torch's index is its own)
            assert bool(torch.equal(flat[live], ti[live])), c.name
        else:
            assert bool(torch.isnan(y.float()).any())
        dy = co.small_ints(y.shape, dtype, co._gen(c.seed + 1))
        dx = co.maxpool_bwd_reference(dy, arg, g)
        assert float(dx.double().abs().max()) < 256
        assert c.fill != "relu" or float(dx.double().sum()) == float(dy.double().sum()), c.name           # every output's gradient lands exactly once
    for n in co.RELU_N[:4]:
        x, gate = co.relu_input(n, dtype, co._gen(n)), co.relu_input(n, dtype, co._gen(n + 1), 3)
        y = co.relu_reference(x)
        t = torch.relu(x.float())
        assert bool(torch.equal(torch.isnan(y), torch.isnan(t))) and bool((y.float()[~torch.isnan(t)] == t[~torch.isnan(t)]).all())
        assert not bool(torch.signbit(y.float()[~torch.isnan(y)]).any())
        yg = co.relu_reference(x, gate)
        on = gate.float() > 0
        assert co.same_bits(yg[on], x[on]) and bool((yg[~on].view(co.INT_VIEW[dtype]) == 0).all())
    x = co.relu_input(64, dtype, co._gen(1))
    assert bool(torch.isnan(x).any()) and bool(torch.isinf(x).any()) and bool(torch.signbit(x.float()[x == 0]).any())
    assert co.same_bits(x, x.clone()) and not co.same_bits(x, -x)


# ------------------------------------------------------------------------------------------------------------------ refusals
_P = 4096                     # a fake, 16-byte aligned device address: every call below is refused before any launch


def test_entry_points_refuse_with_their_documented_codes():
    h = L.lib().cdll
    for dt in co.DTYPES3:
        N, code = co.NVEC[dt], CODE[dt]
        C = N + 1
        assert h.ofa_batchnorm_fwd(_P, _P, _P, None, _P, _P, _P, _P, _P, _P, 4, C, 1e-5, 0.1, 0, 0, code, None) == UNSUPPORTED
        assert h.ofa_batchnorm_fwd(_P, _P, _P, None, _P, _P, _P, None, None, _P, 4, 2 * N, 1e-5, 0.1, 1, 0, code, None) == INVALID   # eval, no running
        assert h.ofa_batchnorm_bwd(_P, _P, _P, _P, _P, _P, _P, None, _P, _P, _P, 4, C, 1, 0, 0, None, code, None) == UNSUPPORTED
        assert h.ofa_batchnorm_bwd(_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, 4, 2 * N, 1, 1, 0, _P, code, None) == INVALID          # beta with dres
        assert h.ofa_batchnorm_bwd_dx(_P, _P, _P, _P, _P, _P, _P, _P, _P, 4, _P, 2 * N, 1, _P, code, None) == INVALID
        assert h.ofa_batchnorm_fwd_stats(_P, _P, _P, 4, C, code, None) == UNSUPPORTED
        assert h.ofa_batchnorm_fwd_apply(_P, _P, _P, None, _P, _P, _P, None, None, _P, 1, 4, C, 1e-5, 0.1, 0, code, None) == UNSUPPORTED
        assert h.ofa_batchnorm_bwd_stats(_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, 4, C, 0, 0, None, code, None) == UNSUPPORTED
        assert h.ofa_maxpool_fwd(_P, _P, _P, 1, 4, 4, C, 3, 2, 1, code, None) == UNSUPPORTED
        assert h.ofa_maxpool_bwd(_P, _P, _P, 1, 4, 4, C, 3, 2, 1, code, None) == UNSUPPORTED
        assert h.ofa_maxpool_fwd(_P, _P, _P, 1, 1, 4, N, 2, 2, 0, code, None) == INVALID                                                # empty output
        assert h.ofa_maxpool_bwd(_P, _P, _P, 1, 1, 4, N, 2, 2, 0, code, None) == INVALID
        assert h.ofa_col2im(_P, _P, 1, 4, 4, C, 3, 3, 1, 1, 16 * C, code, None) == UNSUPPORTED
        assert h.ofa_col2im(_P, _P, 1, 4, 4, N, 3, 3, 1, 1, 9 * N - 8, code, None) == INVALID                                            # Kpad < K
        assert h.ofa_col2im(_P, _P, 1, 1, 4, N, 3, 3, 3, 0, 16 * N, code, None) == INVALID                                               # empty output
        assert h.ofa_im2col(_P, _P, 1, 4, 4, N, 3, 3, 1, 1, 9 * N - 8, 0, code, None) == INVALID                                         # Kpad < K
        assert h.ofa_im2col(_P, _P, 1, 1, 4, N, 3, 3, 3, 0, 16 * N, 0, code, None) == INVALID                                            # empty output
        assert h.ofa_im2col(_P, _P, 1, 2, 2, N, 3, 3, 2, 0, 16 * N, 1, code, None) == INVALID
    assert h.ofa_relu(None, None, None, 5, L.BF16, None) == INVALID and h.ofa_relu(_P, None, _P, 4, 7, None) == INVALID
