"""GPU: every GEMM route (csrc/gemm_mfma.hip, gemm_pp.hip, gemm_core.h, gemm_simple.hip: SIMPLE, REG, LDS_DMA, RING, BIG, PP, MIXED,
split-K + reduce, fold-deferred reduce, two-level batching, column statistics, the grouped launch) per element against a float64 matmul
of small-integer operands, with no tolerance anywhere: only ==, isfinite and isnan.  Cases, operands, reference and checker are those of
tests/gemm_exact.py (regimes, the two 16-bit accumulation contracts, the NaN-poisoned surroundings and their named exceptions are
described there); tests/test_gemm_exact_cpu.py pins every case to the route it covers.  Every call runs twice into fresh NaN outputs.

What each test pins (the gaps the suite had):
  max|a-b| / max|b| over the whole matrix ............. every element == the float64 integer: one dropped or doubled k, a swapped row,
                                                        a bias missing on one quad, a stale LDS stage changes an element by >= 1
  no N % 8 != 0 on an MFMA route ...................... N = 77, 141, 4101, N % 8 == 4 (140, 4100): `second`, N4 slabs, N4 <= ldc
  OFA_GEMM_A_KPAD_ZERO without a kernel-level test .... K = 1000 / 1001 / 8200 / 8201 against A's zero tail, B's rows past K are NaN
  two-level batching only through whole models ........ kernels.gemm_heads: scores, context, value gradient on [B, T, heads * hd] rows
  reads and writes outside the operands ............... NaN around every operand and output: a read that is not clamped gives NaN,
                                                        a store outside [M, N4) replaces one
  two undocumented 16-bit accumulation arithmetics .... the rounding regime with accumulation expects each route's own contract"""
import pytest
import torch

from tests import gemm_exact as G

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
PRODUCTS = sorted({n.rsplit(" ", 1)[0] for n, c in G.CASES.items() if not c.env})


@pytest.fixture(scope="module")
def K():
    from ofasys_amd import kernels
    return kernels


@pytest.mark.parametrize("product", PRODUCTS)
def test_gemm_exact(K, product):
    """Every form of the product (plain, column bias with alpha 0.5, 16-bit and fp32 accumulation, rounding, ...) on the route the
    shipped planner takes for it."""
    for name, case in G.CASES.items():
        if not case.env and name.rsplit(" ", 1)[0] == product:
            G.run_case(K, case, DEV)
    torch.cuda.synchronize()


@pytest.mark.parametrize("group", sorted(G.forced_groups()))
def test_gemm_exact_forced_routes(group):
    """The routes only the debug library's planner overrides reach (OFASYS_AMD_LIB = libofasys_amd_dbg.so, hence the subprocess):
    small -- OFA_GEMM_TILE 11 / 12 / 22 (the 64 x 128 and 128 x 128 ring forms are reachable no other way); big -- OFA_GEMM_TILE 83 / 84
    with OFA_GEMM_PP 0 / 23; mixed -- OFA_GEMM_MIXED=1; split -- OFA_GEMM_SPLIT_MIN_K=256 (read once: a process of its own), split-K on
    every four-wave tile kernel, ring and double-buffered loop, at K = 1100 TN and K = 1024 NN.  Same regimes, poisoned views and checker.
    A child that ends on a signal or the timeout fails the test; it is not run again."""
    r = G.run_child("run", group)
    assert r.returncode == 0 and f"forced ok {len(G.forced_groups()[group])}" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K_,bias,route", G.COLSTAT)
def test_gemm_colstat_exact(K, dtype, M, N, K_, bias, route):
    """ofa_gemm_colstat on exact operands: every partial sum of the column statistics is an integer below 2^24, so part.sum(0) == the
    float64 column sums and sums of squares of the output, and the output == the float64 product.  `route`: the epilogue that writes the
    statistics (ring, 32 rows per partial row; register-staged loop, 64), pinned by test_gemm_exact_cpu.py::test_colstat_route_table."""
    dt = G.DTYPES[dtype]
    g = G._gen("colstat", M, N, K_)
    _, a = G.poisoned(G.int_operand((1, M, K_), "exact", K_, g), G.ceil_to(K_, 8) + 8, dt, DEV)
    _, b = G.poisoned(G.int_operand((1, N, K_), "exact", K_, g), G.ceil_to(K_, 8) + 8, dt, DEV)
    bv = G.poisoned_vec(torch.randint(-3, 4, (N,), generator=g), dt, DEV) if bias else None
    ref = a[0].double() @ b[0].double().t()
    if bias:
        ref = ref + bv.double()
    assert G.representable(ref, dt) and float((ref * ref).sum(0).max()) < 2 ** 24
    want = torch.stack([ref.sum(0), (ref * ref).sum(0)])
    for _ in range(2):
        out, part = K.gemm_colstat(a[0], b[0], bias=bv)
        assert part is not None and part.dtype == torch.float64 and part.shape[1:] == (2, N)
        G.compare(out[None], ref[None], torch.zeros_like(ref[None], dtype=torch.bool), what=f"colstat {M}x{N}x{K_} {dtype} out")
        G.compare(part.sum(0)[None], want[None], torch.zeros_like(want[None], dtype=torch.bool), what=f"colstat {M}x{N}x{K_} {dtype} sums")


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("regime", ["exact", "rounding"])
@pytest.mark.parametrize("path", ["slabs", "direct"])
def test_gemm_group_tn_exact(K, dtype, regime, path):
    """ofa_gemm_group_tn on integer operands; every other dy with lda > m, NaN rows after row k of every dy / x (the ragged contraction
    tail: A's missing rows come from the zero source, B's are clamped).  slabs: fp32 slabs + fold onto an fp32 out; direct: a 16-bit out,
    which a one-slice product reaches in the kernel's epilogue (round, add, round) and a split one through the fold (fp32, one
    rounding).  exact: both == the float64 result; rounding: each product == its own contract.  Rows after out's last row stay NaN."""
    dt = G.DTYPES[dtype]
    odt = torch.float32 if path == "slabs" else dt
    prods, wants = [], []
    for i, ((m, n, k), alpha, splits) in enumerate(zip(G.GROUP, G.GROUP_ALPHA, G.GROUP_SPLITS)):
        g = G._gen("group", m, n, k, regime)
        _, dy = G.poisoned(G.int_operand((1, k, m), regime, k, g), m + 8 * (i % 2), dt, DEV)
        _, x = G.poisoned(G.int_operand((1, k, n), regime, k, g), n + 8 * ((i + 1) % 2), dt, DEV)
        old = torch.randint(-3, 4, (m, n), generator=g).to(DEV).double()
        P = dy[0].double().t() @ x[0].double()
        if regime == "exact":
            exp = alpha * P + old
            for step in (P, alpha * P, exp):
                assert G.representable(step, odt), (m, n, k)
        else:
            assert 9 * k < 2 ** 24
            exp = G.accumulated(alpha * P, old, odt, "round-add-round" if splits == 1 else "fp32-once")
        store = torch.full((m + G.ROW_PAD, n), G.NAN, dtype=odt, device=DEV)
        want = torch.full((1, m + G.ROW_PAD, n), G.NAN, dtype=torch.float64, device=DEV)
        want[0, :m] = exp
        assert K.gemm_group_ok(dy[0], x[0], store[:m])
        prods.append((dy[0], x[0], store[:m], alpha))
        wants.append((store, old, want))
    for _ in range(2):
        for store, old, want in wants:
            store.fill_(G.NAN)
            store[:old.shape[0]] = old
        q = K.FoldQueue()
        K.gemm_group_tn(prods, q)
        assert len(q.jobs) == (len(G.GROUP) if path == "slabs" else sum(s > 1 for s in G.GROUP_SPLITS))
        q.flush()
        for (m, n, k), (store, old, want) in zip(G.GROUP, wants):
            G.compare(store[None], want, torch.zeros_like(want, dtype=torch.bool), (256, 256), f"group {path} {regime} {m}x{n}x{k} {dtype}")
