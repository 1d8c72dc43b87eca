"""GPU: the convolution-stack kernels (csrc/conv.hip: im2col in its three forms, col2im, the BatchNorm statistics / finalize / apply /
backward kernels, MaxPool forward and backward, ReLU) against the oracle of tests/conv_oracle.py.  im2col, col2im, the pools and ReLU are
compared bit for bit; every element of every BatchNorm output within TOL eps of the float64 reference relative to its componentwise
magnitude bound (fp32 tensors and the fp32 statistics: error / bound within 8 x the emulation's).  Every output buffer holds NaN before
the call.

What each test pins (the gaps the suite had):
  max|a-b| / max|b| at 1e-2 ... 3e-2 against torch in fp32 ... per element against float64; mean, rstd, the running buffers and `sums`
  the second sweep of the grid-stride loops ................. bn_apply / bn_bwd_dx (4100 x 256 vectors), col2im, both pools, relu and
                                                              im2col's vector loop, each at 65 x 65 x 256 vectors or 4096 * 256 + 257
  the statistics' pair loop and one-row tail ................ lanes with 0, 1, 2, 3 and >= 5 rows; 256 groups exactly and binding; rows = 1
  bn_fold_groups' second trip, the C % 16 tail .............. 1 ... 513 partial rows behind ofa_batchnorm_fwd_apply; C = 8, 24, 40, 264
  the recomputed ReLU gate .................................. every element of dx, the sums and the parameter gradients: no ambiguous
                                                              element exists (tests/test_conv_oracle_cpu.py)
  accumulate, batch_stats = 0, eval beyond one block, the SyncBatchNorm entry points with total_rows != rows
  im2col: the LDS kernel at 6 / 64 / 65 / 390 positions, its 48 KB hand-over, the NCHW element fallback, the audio stem, the scalar NHWC
          path, pure pad vectors -- the pad columns themselves are compared (+0)
  maxpool: ties in nearly every window, windows of -inf, NaN windows, the arg-max byte, positions no window covers (dx exactly 0)
  NaN through relu and BatchNorm + ReLU ..................... propagates, as torch's
  refusals .................................................. asserted as OfaError, never launched
Run with -s for the worst figure per output and dtype."""
import pytest
import torch

from tests import conv_oracle as co

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
IDS = [co.NAMES[d] for d in co.DTYPES3]
WORST = {}


@pytest.fixture(scope="module")
def cg():
    from tests import conv_gpu
    return conv_gpu


def _bn(cg, dtype, cases):
    worst = WORST.setdefault(co.NAMES[dtype], {})
    for case in cases:
        c = co.build_bn(case, dtype, cg.DEV)
        fig = co.bn_figures(c, cg.run_bn(c), dtype)
        bad = []
        for n, v in fig.items():
            worst[n] = max(worst.get(n, 0.0), v)
            if not v <= co.limit(n, dtype, kernel=True):
                bad.append((n, v, co.limit(n, dtype, kernel=True)))
        assert not bad, (case.name, co.NAMES[dtype], bad)
    print(f"\nbatchnorm {co.NAMES[dtype]}: " + ", ".join(f"{n} {v:.3g}" for n, v in sorted(worst.items())))


@pytest.mark.parametrize("dtype", co.DTYPES3, ids=IDS)
def test_batchnorm_seams_and_flags(cg, dtype):
    """ofa_batchnorm_fwd + _bwd: every cw class, the pair loop and its tail, rows = 1, training / eval, both gate routes and none, dres,
    accumulated gradients, batch_stats = 0, eval at 264 channels, NaN through the fused ReLU; ofa_batchnorm_fwd_apply behind 1 ... 513
    partial rows; the SyncBatchNorm entry points with rows A != rows B."""
    _bn(cg, dtype, [c for c in co.BN_CASES if (c.rows + c.nb) * co.bn_cols(c, dtype) <= co.BIG])


@pytest.mark.parametrize("dtype", co.DTYPES3, ids=IDS)
def test_batchnorm_group_cap_and_second_sweep(cg, dtype):
    """32768 and 32897 rows of 32 vectors (256 row groups exactly, and the cap binding); 4100 rows of 256 vectors: the second trip of
    bn_apply_kernel and bn_bwd_dx_kernel."""
    _bn(cg, dtype, [c for c in co.BN_CASES if (c.rows + c.nb) * co.bn_cols(c, dtype) > co.BIG])


@pytest.mark.parametrize("dtype", co.DTYPES3, ids=IDS)
def test_im2col_routes_bit_exact(cg, dtype):
    """Random finite bit patterns through every im2col route: each element where the stated order puts it, +0 outside the image and in
    the pad columns."""
    for c in co.for_dtype(co.IM2COL_CASES, dtype):
        g = co.case_geom(c, dtype)
        shape = (g.B, g.C, g.H, g.W) if c.nchw else (g.B * g.H * g.W, g.C)
        x = co.random_bits(shape, dtype, co._gen(c.seed)).to(cg.DEV)
        assert co.same_bits(cg.run_im2col(x, g, c.nchw), co.im2col_reference(x, g, c.nchw)), (c.name, co.NAMES[dtype])


@pytest.mark.parametrize("dtype", co.DTYPES3, ids=IDS)
def test_col2im_exact_integers(cg, dtype):
    """Small integers: the sums are exact in any order; positions no window covers are +0 over the NaN fill; one case beyond 4096 blocks."""
    for c in co.COL2IM_CASES:
        g = co.case_geom(c, dtype)
        Ho, Wo = co.geom_out(g)
        dcol = co.small_ints((g.B * Ho * Wo, co.kpad(g)), dtype, co._gen(c.seed)).to(cg.DEV)
        assert co.same_bits(cg.run_col2im(dcol, g), co.col2im_reference(dcol, g)), (c.name, co.NAMES[dtype])


@pytest.mark.parametrize("dtype", co.DTYPES3, ids=IDS)
def test_maxpool_ties_nan_and_backward(cg, dtype):
    """y and the arg-max byte bit for bit on maps that tie in nearly every window (a post-ReLU map, windows of -inf, NaN windows); the
    backward on the oracle's taps with integer gradients, exactly 0 where no window reaches; one case beyond 4096 blocks each way."""
    for c in co.MAXPOOL_CASES:
        g = co.case_geom(c, dtype)
        x = co.pool_input(c, g, dtype, co._gen(c.seed)).to(cg.DEV)
        y, arg = cg.run_maxpool(x, g)
        ry, rarg = co.maxpool_reference(x, g)
        assert co.same_bits(y, ry) and co.same_bits(arg, rarg), (c.name, co.NAMES[dtype])
        dy = co.small_ints(ry.shape, dtype, co._gen(c.seed + 1)).to(cg.DEV)
        assert co.same_bits(cg.run_maxpool_bwd(dy, rarg, g), co.maxpool_bwd_reference(dy, rarg, g)), (c.name, co.NAMES[dtype])


@pytest.mark.parametrize("dtype", co.DTYPES3, ids=IDS)
def test_relu_specials_and_second_sweep(cg, dtype):
    """+-0, +-smallest subnormal, +-inf, NaN among normal values at 1, 255, 256, 257 and 4096 * 256 + 257 elements, forward and gated:
    NaN propagates through the forward form; a NaN, zero or negative gate closes."""
    for n in co.RELU_N:
        x = co.relu_input(n, dtype, co._gen(n)).to(cg.DEV)
        gate = co.relu_input(n, dtype, co._gen(n + 1), 3).to(cg.DEV)
        assert co.same_bits(cg.run_relu(x), co.relu_reference(x)), (n, co.NAMES[dtype], "forward")
        assert co.same_bits(cg.run_relu(x, gate), co.relu_reference(x, gate)), (n, co.NAMES[dtype], "gated")


def test_refusals_raise_before_any_launch(cg):
    """C that is no whole number of vectors (BatchNorm, the pools, col2im), Kpad < K, an empty output, eval mode without running
    statistics, beta together with dres: OfaError, and the output buffers still hold their NaN."""
    from ofasys_amd.lib import OfaError
    for dtype in co.DTYPES3:
        N = co.NVEC[dtype]
        code = cg.CODE[dtype]
        t = lambda *s: torch.ones(*s, dtype=dtype, device=cg.DEV)           # noqa: E731
        f = lambda *s: torch.ones(*s, dtype=torch.float32, device=cg.DEV)   # noqa: E731
        C = N + 1
        y = cg.nan((4, 2 * N), dtype)
        with pytest.raises(OfaError, match="multiple of"):
            cg._call("ofa_batchnorm_fwd", t(4, C), t(C), t(C), None, y, f(C), f(C), f(C), f(C), cg.ws_for(C), 4, C, 1e-5, 0.1, 0, 0, code)
        with pytest.raises(OfaError, match="running statistics"):
            cg._call("ofa_batchnorm_fwd", t(4, 2 * N), t(2 * N), t(2 * N), None, y, f(2 * N), f(2 * N), None, None, cg.ws_for(2 * N), 4, 2 * N,
                     1e-5, 0.1, 1, 0, code)
        with pytest.raises(OfaError, match="recomputed"):
            cg._call("ofa_batchnorm_bwd", t(4, 2 * N), None, t(4, 2 * N), t(2 * N), f(2 * N), f(2 * N), y, cg.nan((4, 2 * N), dtype), t(2 * N),
                     t(2 * N), cg.ws_for(2 * N), 4, 2 * N, 1, 1, 0, t(2 * N), code)
        with pytest.raises(OfaError, match="multiple of"):
            cg._call("ofa_maxpool_fwd", t(16, C), y, torch.zeros(64, dtype=torch.uint8, device=cg.DEV), 1, 4, 4, C, 3, 2, 1, code)
        with pytest.raises(OfaError, match="empty output"):
            cg._call("ofa_maxpool_fwd", t(4, N), y, torch.zeros(64, dtype=torch.uint8, device=cg.DEV), 1, 1, 4, N, 2, 2, 0, code)
        with pytest.raises(OfaError, match="multiples of"):
            cg._call("ofa_col2im", t(16, 16 * C), y, 1, 4, 4, C, 3, 3, 1, 1, 16 * C, code)
        with pytest.raises(OfaError, match="bad argument"):
            cg._call("ofa_im2col", t(16, N), y, 1, 4, 4, N, 3, 3, 1, 1, 9 * N - 8, 0, code)
        with pytest.raises(OfaError, match="empty output"):
            cg._call("ofa_im2col", t(4, N), y, 1, 1, 4, N, 3, 3, 3, 0, 16 * N, 0, code)
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all())
