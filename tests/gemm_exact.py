"""The GEMM family (csrc/gemm_mfma.hip, gemm_pp.hip, gemm_core.h, gemm_simple.hip) pinned per element with exact integer products:
the case table, the operands, the float64 reference and the checker shared by tests/test_gemm_exact_cpu.py and
tests/test_gemm_exact_gpu.py.  Importing this module needs no GPU and does not load the library.

With small-integer operands every product and every partial sum of a GEMM with fp32 accumulation is an exactly representable fp32
integer in any summation order, so every route, tile shape, K-split and reduce must return exactly what a float64 matmul returns:
no tolerance anywhere, only ==, isfinite and isnan.

Regimes (the case builder asserts their preconditions on the float64 reference alone; they are conditions, not measurements)
  exact ...... operands i.i.d. in {-1, 0, 1} (K > 4160: non-zeros thinned to 1/3 per operand), bias and the old C integers in -3 .. 3,
               alpha in {1, 0.5, -2}.  Precondition: the float64 value of every step -- the product P, (P + bias) * alpha, + C -- is
               exactly representable in the output type.  Then nothing is rounded anywhere and both 16-bit accumulation arithmetics
               give the same bits.
  rounding ... operands dense in -3 .. 3.  Precondition: 9 K < 2^24, so every partial sum is an exact fp32 integer.  Expected: the
               float64 value rounded ONCE to the output type, to nearest even (bf16 integers above 256 sit on exact ties all the time:
               enc2's tie rule on every route).

The two 16-bit accumulation contracts (OFA_GEMM_ACCUM onto a 16-bit C; include/ofasys_amd.h at ofa_gemm), which the rounding regime
tells apart:
  round-add-round ... the tile kernels' own epilogue (epilogue_lds, acc16) and the grouped launch's direct path round the tile to 16
                      bits, add the old C and round again: C = rn16(rn16(alpha (P + bias)) + C_old);
  fp32-once ......... a split-K product finished by the reduce launch or by the fold (epilogue_store, fold.hip) and the exact kernel
                      (gemm_simple_kernel) add the old C in fp32 and round once: C = rn16(alpha (P + bias) + C_old).
contract_of() reads the contract off the case's route string.

Poisoned surroundings.  Every operand is a view into wider storage filled with NaN: rows after the operand's last row (for an m-major
operand these are the k rows past K), the columns between its logical width and the leading dimension.  The output is a view inside
NaN storage [M + 8, ldc], ldc > N4 = (N + 3) & ~3.  Reading NaN is no fault; a kernel that reads where it should clamp, or reads
zeros from the wrong place, turns an output into NaN.  The exceptions, each named in its case's `exceptions`:
  KPAD_ZERO_TAIL ... A[:, K : lda) holds zeros: that IS the contract of OFA_GEMM_A_KPAD_ZERO (the kernels run the contraction over K
                     rounded up to whole tiles and rely on 0 x B[clamped row]).
  FOLD_DENSE_OUT ... a fold-deferred product writes C through the FoldQueue, which takes a contiguous output with N % 4 == 0
                     (kernels.gemm defers only then): ldc == N, the poison is the rows >= M alone.
  HEADS_S_PAD ...... scores of kernels.gemm_heads are stored [B heads, T, S padded to 80]: ldc == N4 == 80 as the model stores them.

Checker, per element of the whole output storage: inside [M, N] finite and == expected; rows >= M and columns >= N4 still NaN;
columns [N, N4) unspecified (the kernels may write the rest of the last quad) -- the only region not compared.
"""
import dataclasses
import functools
import re
import zlib

import torch

NT, NN, TN, TT = (0, 1), (0, 0), (1, 0), (1, 1)
LAYOUT_NAMES = {NT: "NT", NN: "NN", TN: "TN", TT: "TT"}
BIAS_COL, BIAS_ROW, ACCUM, OUT_F32, A_KPAD_ZERO, DEFER_REDUCE = 1, 2, 4, 16, 32, 128      # ofa_gemm.flags
WS = 256 << 20                                                                               # kernels.gemm's workspace
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
DTYPE_CODES = {"f32": 0, "bf16": 1, "f16": 2}                                                # ofasys_amd.lib.F32 / BF16 / F16
NAN = float("nan")
ROW_PAD = 8                   # NaN rows after every operand and output
KPAD_ZERO_TAIL, FOLD_DENSE_OUT, HEADS_S_PAD = "KPAD_ZERO_TAIL", "FOLD_DENSE_OUT", "HEADS_S_PAD"


def ceil_to(n, q):
    return (n + q - 1) // q * q


def cdiv(a, b):
    return (a + b - 1) // b


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    layout: tuple
    regime: str = "exact"            # "exact" | "rounding"
    dtype: str = "bf16"              # operand type
    bias: str = ""                   # "" | "col" | "row"
    alpha: float = 1.0
    accumulate: bool = False
    out_f32: bool = False
    a_kpad_zero: bool = False
    fold: bool = False               # fold-deferred reduce (fold=FoldQueue())
    batch: int = 1
    heads: tuple = ()                # (B, heads, product) for kernels.gemm_heads: product in "scores" | "context" | "dvalue"
    lda: int = 0                     # 0: the default of default_ld()
    ldb: int = 0
    ldc: int = 0
    unaligned: bool = False          # odd leading dimensions: no MFMA kernel takes the call (SIMPLE)
    twin: tuple = ()                 # (M, N, K): the dense product the launch plans when the case is a view
    env: tuple = ()                  # ((name, value), ...): planner overrides of the debug library (forced routes)
    exceptions: tuple = ()

    @property
    def flags(self):
        f = {"": 0, "col": BIAS_COL, "row": BIAS_ROW}[self.bias]
        f |= ACCUM if self.accumulate else 0
        f |= OUT_F32 if (self.out_f32 and self.dtype != "f32") else 0
        f |= A_KPAD_ZERO if self.a_kpad_zero else 0
        f |= DEFER_REDUCE if self.fold else 0
        return f

    @property
    def out_dtype(self):
        return torch.float32 if (self.out_f32 or self.dtype == "f32") else DTYPES[self.dtype]

    @property
    def N4(self):
        return (self.N + 3) & ~3

    @property
    def nbatch(self):
        return self.heads[0] * self.heads[1] if self.heads else self.batch

    def plan_args(self):
        """(M, N, K, layout, flags, dtype code, batch, workspace) for ofa_gemm_plan: the case itself, or its plan twin."""
        M, N, K = self.twin or (self.M, self.N, self.K)
        return M, N, K, self.layout, self.flags, DTYPE_CODES[self.dtype], self.nbatch, WS


# ------------------------------------------------------------------ the case table
def _variants(tag, M, N, K, layout, batch=1, dtype="bf16", which=("plain", "bias", "acc16", "acc32", "rounding"), **kw):
    """The five forms every listed product runs in."""
    base = f"{tag} {M}x{N}x{K} {LAYOUT_NAMES[layout]}" + (f" batch {batch}" if batch > 1 else "") + f" {dtype}"
    forms = {
        "plain": dict(),
        "bias": dict(bias="col", alpha=0.5),
        "acc16": dict(accumulate=True),
        "acc32": dict(accumulate=True, out_f32=True),
        "rounding": dict(regime="rounding"),
        "rowbias": dict(bias="row", alpha=-2.0),
        "round_acc16": dict(regime="rounding", accumulate=True),
        "round_bias": dict(regime="rounding", bias="col", alpha=0.5),
    }
    return [Case(name=f"{base} {w}", M=M, N=N, K=K, layout=layout, batch=batch, dtype=dtype, **{**forms[w], **kw}) for w in which]


def _cases():
    c = []
    # ---- routes the shipped planner takes at small shapes
    for lay in (NT, NN, TN, TT):
        c += _variants("SIMPLE", 70, 77, 200, lay, unaligned=True)
    c += _variants("SIMPLE", 70, 77, 200, NT, unaligned=True, which=("round_acc16",))
    c += _variants("SIMPLE", 70, 77, 200, NT, dtype="f32", unaligned=True, which=("plain", "bias", "acc32"))
    c += _variants("SIMPLE", 70, 77, 200, TN, dtype="f16", unaligned=True, which=("plain", "rounding"))
    for M, N, K, lay, b in [(70, 76, 200, NT, 1), (72, 80, 200, NN, 1), (72, 76, 200, TT, 1), (200, 264, 1000, NN, 1), (70, 64, 72, NN, 12)]:
        c += _variants("REG", M, N, K, lay, b)
    c += _variants("REG", 70, 76, 200, NT, dtype="f16")
    c += _variants("REG", 72, 80, 200, NN, which=("round_acc16",))
    for M, N, K, lay, b in [(600, 520, 192, NT, 1), (2100, 1032, 192, NN, 1), (264, 200, 40, TN, 1), (520, 520, 100, TN, 1),
                            (100, 76, 64, NT, 6), (72, 64, 70, TN, 12), (3000, 1500, 256, NT, 1), (1800, 2048, 1100, TN, 1)]:
        c += _variants("LDS_DMA", M, N, K, lay, b)
    c += _variants("LDS_DMA", 600, 520, 192, NT, dtype="f16")
    c += _variants("LDS_DMA", 600, 520, 192, NT, which=("rowbias", "round_acc16", "round_bias"))
    for M, N, K, lay, b in [(520, 520, 4100, TN, 1), (1032, 520, 2048, NN, 1), (264, 264, 2100, TN, 4)]:
        c += _variants("LDS_DMA split", M, N, K, lay, b)
    c += _variants("LDS_DMA split", 520, 520, 4100, TN, dtype="f16")
    c += _variants("LDS_DMA split", 520, 520, 4100, TN, which=("rowbias", "round_acc16"))
    for M, N, K, lay, b in [(136, 140, 256, NT, 1), (200, 264, 1024, NN, 1), (264, 200, 1025, TN, 1), (1000, 520, 256, NT, 1),
                            (200, 264, 256, NN, 3)]:
        c += _variants("RING", M, N, K, lay, b)
    c += _variants("RING", 136, 140, 256, NT, dtype="f16")
    c += _variants("RING", 136, 140, 256, NT, which=("round_acc16",))
    c += _variants("RING", 200, 264, 1024, NN, which=("round_acc16",))          # (K long enough that most entries pass 256: the two
    c += _variants("LDS_DMA", 1800, 2048, 1100, TN, which=("round_acc16",))     #  accumulation contracts differ in hundreds of elements)
    for M, N, K, lay in [(392, 520, 2100, TN), (200, 140, 8192, NT)]:
        c += _variants("RING split", M, N, K, lay)
    c += _variants("RING split", 392, 520, 2100, TN, dtype="f16", which=("plain", "acc16", "rounding"))
    c += _variants("RING split", 392, 520, 2100, TN, which=("round_acc16",))
    for M, N, K, lay in [(2900, 4100, 256, NT), (4500, 2100, 256, NT)]:
        c += _variants("BIG", M, N, K, lay)
    c += _variants("BIG", 4500, 2100, 256, NT, dtype="f16", which=("plain", "rounding"))
    c += _variants("BIG", 4500, 2100, 256, NT, which=("round_acc16",))
    for M, N, K, lay in [(4500, 2104, 2048, NN), (2900, 4104, 2048, NN), (3600, 3592, 1088, TN)]:
        c += _variants("PP", M, N, K, lay)
    c += _variants("PP", 3600, 3592, 1088, TN, dtype="f16", which=("plain", "rounding"))
    c += _variants("PP", 3600, 3592, 1088, TN, which=("round_acc16",))
    for M, N, K, lay in [(448, 520, 8192, NT), (200, 264, 8256, NN)]:
        c += _variants("big split", M, N, K, lay)
    c += _variants("big split", 200, 264, 8256, NN, dtype="f16", which=("plain", "rounding"))
    # ---- views, each with its plan twin
    for K, lda in [(1000, 1024), (1001, 1024), (8200, 8256), (8201, 8256)]:
        c += _variants("view kpad", 200, 264, K, NN, which=("plain", "bias", "acc16", "rounding"), a_kpad_zero=True, lda=lda,
                       twin=(200, 264, lda), exceptions=(KPAD_ZERO_TAIL,))
    ragged = [("REG", 70, 77, 200, NT), ("REG", 70, 141, 200, NT), ("REG", 72, 77, 200, NN), ("REG", 72, 141, 200, NN),
              ("LDS_DMA", 600, 77, 192, NT), ("LDS_DMA", 600, 141, 192, NT), ("LDS_DMA", 600, 77, 192, NN), ("LDS_DMA", 600, 141, 192, NN),
              ("LDS_DMA", 264, 77, 40, TN), ("LDS_DMA", 264, 141, 40, TN),
              ("RING", 136, 77, 256, NT), ("RING", 136, 141, 256, NT), ("RING", 200, 77, 1024, NN), ("RING", 200, 141, 1024, NN),
              ("RING", 264, 77, 1025, TN), ("RING", 264, 141, 1025, TN), ("RING", 1000, 77, 256, NT),
              # (a big tile needs N >= 256: the same raggedness, N % 8 == 5, on 4101 columns)
              ("BIG", 2900, 4101, 256, NT), ("PP", 2900, 4101, 2048, NN),
              # split-K: the fp32 slabs have row stride N4
              ("RING split", 392, 141, 2100, TN), ("RING split", 392, 77, 2048, NN), ("RING split", 200, 141, 8192, NT)]
    for tag, M, N, K, lay in ragged:
        ldb = 0 if lay[1] else ceil_to(N, 8)                 # m-major B: ldb = ceil8(N), the last vector ends on the row's end
        c += _variants("view ragged N " + tag, M, N, K, lay, which=("plain", "acc16", "acc32", "rounding"), ldb=ldb, ldc=((N + 3) & ~3) + 8,
                       twin=(M, ceil_to(N, 8), K))
    # the fold-deferred form (FoldQueue): N % 8 == 4.  kernels.gemm defers only onto a contiguous C with N % 4 == 0, so here the slab row
    # stride N4 equals N: a slab stride N4 != N is exercised by the +reduce cases above only, never through the fold.
    c += _variants("view fold-deferred", 392, 140, 2100, TN, which=("plain", "acc16", "acc32", "rounding", "round_acc16"), fold=True,
                   ldc=140, twin=(392, 144, 2100), exceptions=(FOLD_DENSE_OUT,))
    c += _variants("view fold-deferred", 200, 140, 8192, NT, which=("plain", "acc32"), fold=True, ldc=140, exceptions=(FOLD_DENSE_OUT,))
    # two-level batching: kernels.gemm_heads, B = 2, heads = 3, hd = 64, T = 70, S = 77 stored padded to 80
    for which in ("plain", "rounding"):
        c += _variants("heads scores", 70, 77, 64, NT, which=(which,), heads=(2, 3, "scores"), ldc=80, twin=(70, 80, 64),
                       exceptions=(HEADS_S_PAD,))
        c += _variants("heads context", 70, 64, 77, NN, which=(which,), heads=(2, 3, "context"), lda=80)      # (K % 8: the exact kernel)
        c += _variants("heads context", 70, 64, 80, NN, which=(which,), heads=(2, 3, "context"), lda=80)
        c += _variants("heads dvalue", 77, 64, 70, TN, which=(which,), heads=(2, 3, "dvalue"), lda=80, twin=(80, 64, 70))
    c += _variants("heads dvalue", 77, 64, 70, TN, which=("acc16", "round_acc16"), heads=(2, 3, "dvalue"), lda=80, twin=(80, 64, 70))
    # ---- forced routes (debug library, subprocess)
    for tile in ("11", "12", "22"):
        env = (("OFA_GEMM_TILE", tile),)
        for M, N, K, lay in [(136, 140, 256, NT), (200, 264, 1024, NN), (264, 200, 1025, TN), (600, 520, 192, NT), (70, 76, 200, NT)]:
            c += _variants(f"forced tile {tile}", M, N, K, lay, which=("plain", "bias", "acc16", "rounding"), env=env)
    for tile in ("83", "84"):
        for pp in ("0", "23"):
            env = (("OFA_GEMM_TILE", tile), ("OFA_GEMM_PP", pp))
            for M, N, K in [(600, 520, 192), (192, 256, 64), (1000, 768, 320)]:
              for lay in (NT, NN, TN):                     # every shape in every layout, as test_gemm_eight_wave_tiles_forced does
                c += _variants(f"forced tile {tile} pp {pp}", M, N, K, lay, which=("plain", "bias", "acc16", "rounding"), env=env)
    for lay in (NT, NN):
        c += _variants("forced mixed", 1100, 520, 1024, lay, which=("plain", "bias", "acc16", "acc32", "rounding"), env=(("OFA_GEMM_MIXED", "1"),))
    # split-K on every four-wave tile kernel: the small grids stay on the ring (gemm_ring_kernel), the larger ones -- tiles x slices
    # above 512 (64 x 64) or 256 (wider tiles) -- leave it for gemm_mfma_kernel (LDS_DMA), which the shipped planner never splits at
    # 64 x 64.  A k-major A is only split while its 64 x 64 tiles number < 256, hence one NN shape per tile.  (A forced big tile is never
    # split: gemm_plan splits it only from K = 8192 up, unforced -- the `big split` cases.)
    split_shapes = {"11": [(1032, 1032, 1100, TN), (800, 872, 1024, NN)], "12": [(1032, 1032, 1100, TN), (800, 872, 1024, NN)],
                    "22": [(1032, 1032, 1100, TN), (1025, 904, 1024, NN)]}
    for tile in ("11", "12", "22"):
        env = (("OFA_GEMM_SPLIT_MIN_K", "256"), ("OFA_GEMM_TILE", tile))
        for M, N, K, lay in [(264, 264, 1100, TN), (200, 264, 1024, NN)] + split_shapes[tile]:
            c += _variants(f"forced split tile {tile}", M, N, K, lay, which=("plain", "acc16", "rounding"), env=env)
    names = [x.name for x in c]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return {x.name: x for x in c}


CASES = _cases()


def plan_twin_ok(case):
    """A view's twin rounds K up to 64 (a_kpad_zero), N up to 8 (ragged N) or the M of an m-major A up to 8 (its rows are stored with
    lda = ceil8(M)) and nothing else, and leaves every tile count unchanged."""
    if not case.twin:
        return True
    M, N, K = case.twin
    ok = all(cdiv(N, t) == cdiv(case.N, t) for t in (64, 128, 256)) and all(cdiv(M, t) == cdiv(case.M, t) for t in (64, 128, 192, 256))
    ok = ok and (K == ceil_to(case.K, 64) if case.a_kpad_zero else K == case.K) and N in (case.N, ceil_to(case.N, 8))
    return ok and (M == case.M or (case.layout[0] == 1 and M == ceil_to(case.M, 8)))


# ------------------------------------------------------------------ expected routes (ofa_gemm_plan, tests/test_gemm_plan_cpu.describe)
# product (the case name without its form) -> route of every form; a form whose flags move the plan is listed by its full name.
ROUTES_BY_PRODUCT = {
    'SIMPLE 70x77x200 NT bf16': 'SIMPLE why=3',
    'SIMPLE 70x77x200 NN bf16': 'SIMPLE why=3',
    'SIMPLE 70x77x200 TN bf16': 'SIMPLE why=3',
    'SIMPLE 70x77x200 TT bf16': 'SIMPLE why=3',
    'SIMPLE 70x77x200 NT f32': 'SIMPLE why=1',
    'SIMPLE 70x77x200 TN f16': 'SIMPLE why=3',
    'REG 70x76x200 NT bf16': 'REG 64x64 waves 1x1 of 2x2 K=200 colstat=64',
    'REG 72x80x200 NN bf16': 'REG 64x64 waves 1x1 of 2x2 K=200 colstat=64',
    'REG 72x76x200 TT bf16': 'REG 64x64 waves 1x1 of 2x2 K=200 colstat=64',
    'REG 200x264x1000 NN bf16': 'REG 64x64 waves 1x1 of 2x2 K=1000 colstat=64',
    'REG 70x64x72 NN batch 12 bf16': 'REG 64x64 waves 1x1 of 2x2 K=72 colstat=0',
    'REG 70x76x200 NT f16': 'REG 64x64 waves 1x1 of 2x2 K=200 colstat=64',
    'LDS_DMA 600x520x192 NT bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=192 colstat=64',
    'LDS_DMA 2100x1032x192 NN bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=192 colstat=64',
    'LDS_DMA 264x200x40 TN bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=64 colstat=64',
    'LDS_DMA 520x520x100 TN bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=128 colstat=64',
    'LDS_DMA 100x76x64 NT batch 6 bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=64 colstat=0',
    'LDS_DMA 72x64x70 TN batch 12 bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=128 colstat=0',
    'LDS_DMA 3000x1500x256 NT bf16': 'LDS_DMA 64x128 waves 1x2 of 2x2 K=256 colstat=64',
    'LDS_DMA 1800x2048x1100 TN bf16': 'LDS_DMA 64x128 waves 1x2 of 2x2 K=1152 colstat=64',
    'LDS_DMA 600x520x192 NT f16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=192 colstat=64',
    'LDS_DMA split 520x520x4100 TN bf16': 'LDS_DMA 128x128 waves 2x2 of 2x2 K=4160 splits=13x320 +reduce colstat=0',
    'LDS_DMA split 1032x520x2048 NN bf16': 'LDS_DMA 64x128 waves 1x2 of 2x2 K=2048 splits=5x448 +reduce colstat=0',
    'LDS_DMA split 264x264x2100 TN batch 4 bf16': 'LDS_DMA 64x128 waves 1x2 of 2x2 K=2112 splits=7x320 +reduce colstat=0',
    'LDS_DMA split 520x520x4100 TN f16': 'LDS_DMA 128x128 waves 2x2 of 2x2 K=4160 splits=13x320 +reduce colstat=0',
    'RING 136x140x256 NT bf16': 'RING 64x64 waves 2x2 of 1x1 K=256 colstat=32',
    'RING 200x264x1024 NN bf16': 'RING 64x64 waves 2x2 of 1x1 K=1024 colstat=32',
    'RING 264x200x1025 TN bf16': 'RING 64x64 waves 2x2 of 1x1 K=1088 colstat=32',
    'RING 1000x520x256 NT bf16': 'RING 64x64 waves 2x2 of 1x1 K=256 colstat=32',
    'RING 200x264x256 NN batch 3 bf16': 'RING 64x64 waves 2x2 of 1x1 K=256 colstat=0',
    'RING 136x140x256 NT f16': 'RING 64x64 waves 2x2 of 1x1 K=256 colstat=32',
    'RING split 392x520x2100 TN bf16': 'RING 64x64 waves 2x2 of 1x1 K=2112 splits=7x320 +reduce colstat=0',
    'RING split 200x140x8192 NT bf16': 'RING 64x64 waves 2x2 of 1x1 K=8192 splits=32x256 +reduce colstat=0',
    'RING split 392x520x2100 TN f16': 'RING 64x64 waves 2x2 of 1x1 K=2112 splits=7x320 +reduce colstat=0',
    'BIG 2900x4100x256 NT bf16': 'BIG 256x256 waves 2x4 of 4x2 K=256 colstat=128',
    'BIG 4500x2100x256 NT bf16': 'BIG 192x256 waves 2x4 of 3x2 K=256 colstat=96',
    'BIG 4500x2100x256 NT f16': 'BIG 192x256 waves 2x4 of 3x2 K=256 colstat=96',
    'PP 4500x2104x2048 NN bf16': 'PP 192x256 waves 2x4 of 3x2 K=2048 colstat=96',
    'PP 2900x4104x2048 NN bf16': 'PP 256x256 waves 2x4 of 4x2 K=2048 colstat=128',
    'PP 3600x3592x1088 TN bf16': 'PP 256x256 waves 2x4 of 4x2 K=1088 colstat=128',
    'PP 3600x3592x1088 TN f16': 'PP 256x256 waves 2x4 of 4x2 K=1088 colstat=128',
    'big split 448x520x8192 NT bf16': 'BIG 256x256 waves 2x4 of 4x2 K=8192 splits=32x256 +reduce colstat=0',
    'big split 200x264x8256 NN bf16': 'PP 256x256 waves 2x4 of 4x2 K=8256 splits=26x320 +reduce colstat=0',
    'big split 200x264x8256 NN f16': 'PP 256x256 waves 2x4 of 4x2 K=8256 splits=26x320 +reduce colstat=0',
    'view kpad 200x264x1000 NN bf16': 'RING 64x64 waves 2x2 of 1x1 K=1024 colstat=32',
    'view kpad 200x264x1001 NN bf16': 'RING 64x64 waves 2x2 of 1x1 K=1024 colstat=32',
    'view kpad 200x264x8200 NN bf16': 'PP 256x256 waves 2x4 of 4x2 K=8256 splits=26x320 +reduce colstat=0',
    'view kpad 200x264x8201 NN bf16': 'PP 256x256 waves 2x4 of 4x2 K=8256 splits=26x320 +reduce colstat=0',
    'view ragged N REG 70x77x200 NT bf16': 'REG 64x64 waves 1x1 of 2x2 K=200 colstat=64',
    'view ragged N REG 70x141x200 NT bf16': 'REG 64x64 waves 1x1 of 2x2 K=200 colstat=64',
    'view ragged N REG 72x77x200 NN bf16': 'REG 64x64 waves 1x1 of 2x2 K=200 colstat=64',
    'view ragged N REG 72x141x200 NN bf16': 'REG 64x64 waves 1x1 of 2x2 K=200 colstat=64',
    'view ragged N LDS_DMA 600x77x192 NT bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=192 colstat=64',
    'view ragged N LDS_DMA 600x141x192 NT bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=192 colstat=64',
    'view ragged N LDS_DMA 600x77x192 NN bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=192 colstat=64',
    'view ragged N LDS_DMA 600x141x192 NN bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=192 colstat=64',
    'view ragged N LDS_DMA 264x77x40 TN bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=64 colstat=64',
    'view ragged N LDS_DMA 264x141x40 TN bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=64 colstat=64',
    'view ragged N RING 136x77x256 NT bf16': 'RING 64x64 waves 2x2 of 1x1 K=256 colstat=32',
    'view ragged N RING 136x141x256 NT bf16': 'RING 64x64 waves 2x2 of 1x1 K=256 colstat=32',
    'view ragged N RING 200x77x1024 NN bf16': 'RING 64x64 waves 2x2 of 1x1 K=1024 colstat=32',
    'view ragged N RING 200x141x1024 NN bf16': 'RING 64x64 waves 2x2 of 1x1 K=1024 colstat=32',
    'view ragged N RING 264x77x1025 TN bf16': 'RING 64x64 waves 2x2 of 1x1 K=1088 colstat=32',
    'view ragged N RING 264x141x1025 TN bf16': 'RING 64x64 waves 2x2 of 1x1 K=1088 colstat=32',
    'view ragged N RING 1000x77x256 NT bf16': 'RING 64x64 waves 2x2 of 1x1 K=256 colstat=32',
    'view ragged N BIG 2900x4101x256 NT bf16': 'BIG 256x256 waves 2x4 of 4x2 K=256 colstat=128',
    'view ragged N PP 2900x4101x2048 NN bf16': 'PP 256x256 waves 2x4 of 4x2 K=2048 colstat=128',
    'view ragged N RING split 392x141x2100 TN bf16': 'RING 64x64 waves 2x2 of 1x1 K=2112 splits=7x320 +reduce colstat=0',
    'view ragged N RING split 392x77x2048 NN bf16': 'RING 64x64 waves 2x2 of 1x1 K=2048 splits=8x256 +reduce colstat=0',
    'view ragged N RING split 200x141x8192 NT bf16': 'RING 64x64 waves 2x2 of 1x1 K=8192 splits=32x256 +reduce colstat=0',
    'view fold-deferred 392x140x2100 TN bf16': 'RING 64x64 waves 2x2 of 1x1 K=2112 splits=7x320 colstat=0',
    'view fold-deferred 200x140x8192 NT bf16': 'RING 64x64 waves 2x2 of 1x1 K=8192 splits=32x256 colstat=0',
    'heads scores 70x77x64 NT bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=64 colstat=0',
    'heads context 70x64x77 NN bf16': 'SIMPLE why=3',
    'heads context 70x64x80 NN bf16': 'REG 64x64 waves 1x1 of 2x2 K=80 colstat=0',
    'heads dvalue 77x64x70 TN bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=128 colstat=0',
    'forced tile 11 136x140x256 NT bf16': 'RING 64x64 waves 2x2 of 1x1 K=256 colstat=32',
    'forced tile 11 200x264x1024 NN bf16': 'RING 64x64 waves 2x2 of 1x1 K=1024 colstat=32',
    'forced tile 11 264x200x1025 TN bf16': 'RING 64x64 waves 2x2 of 1x1 K=1088 colstat=32',
    'forced tile 11 600x520x192 NT bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=192 colstat=64',
    'forced tile 11 70x76x200 NT bf16': 'REG 64x64 waves 1x1 of 2x2 K=200 colstat=64',
    'forced tile 12 136x140x256 NT bf16': 'RING 64x128 waves 2x2 of 1x2 K=256 colstat=32',
    'forced tile 12 200x264x1024 NN bf16': 'RING 64x128 waves 2x2 of 1x2 K=1024 colstat=32',
    'forced tile 12 264x200x1025 TN bf16': 'RING 64x128 waves 2x2 of 1x2 K=1088 colstat=32',
    'forced tile 12 600x520x192 NT bf16': 'LDS_DMA 64x128 waves 1x2 of 2x2 K=192 colstat=64',
    'forced tile 12 70x76x200 NT bf16': 'REG 64x128 waves 1x2 of 2x2 K=200 colstat=64',
    'forced tile 22 136x140x256 NT bf16': 'RING 128x128 waves 2x2 of 2x2 K=256 colstat=64',
    'forced tile 22 200x264x1024 NN bf16': 'RING 128x128 waves 2x2 of 2x2 K=1024 colstat=64',
    'forced tile 22 264x200x1025 TN bf16': 'RING 128x128 waves 2x2 of 2x2 K=1088 colstat=64',
    'forced tile 22 600x520x192 NT bf16': 'LDS_DMA 128x128 waves 2x2 of 2x2 K=192 colstat=64',
    'forced tile 22 70x76x200 NT bf16': 'REG 128x128 waves 2x2 of 2x2 K=200 colstat=64',
    'forced tile 83 pp 0 600x520x192 NT bf16': 'BIG 192x256 waves 2x4 of 3x2 K=192 colstat=96',
    'forced tile 83 pp 0 600x520x192 NN bf16': 'BIG 192x256 waves 2x4 of 3x2 K=192 colstat=96',
    'forced tile 83 pp 0 600x520x192 TN bf16': 'BIG 256x256 waves 2x4 of 4x2 K=192 colstat=128',
    'forced tile 83 pp 0 192x256x64 NT bf16': 'BIG 192x256 waves 2x4 of 3x2 K=64 colstat=96',
    'forced tile 83 pp 0 192x256x64 NN bf16': 'BIG 192x256 waves 2x4 of 3x2 K=64 colstat=96',
    'forced tile 83 pp 0 192x256x64 TN bf16': 'BIG 256x256 waves 2x4 of 4x2 K=64 colstat=128',
    'forced tile 83 pp 0 1000x768x320 NT bf16': 'BIG 192x256 waves 2x4 of 3x2 K=320 colstat=96',
    'forced tile 83 pp 0 1000x768x320 NN bf16': 'BIG 192x256 waves 2x4 of 3x2 K=320 colstat=96',
    'forced tile 83 pp 0 1000x768x320 TN bf16': 'BIG 256x256 waves 2x4 of 4x2 K=320 colstat=128',
    'forced tile 83 pp 23 600x520x192 NT bf16': 'PP 192x256 waves 2x4 of 3x2 K=192 colstat=96',
    'forced tile 83 pp 23 600x520x192 NN bf16': 'PP 192x256 waves 2x4 of 3x2 K=192 colstat=96',
    'forced tile 83 pp 23 600x520x192 TN bf16': 'PP 256x256 waves 2x4 of 4x2 K=192 colstat=128',
    'forced tile 83 pp 23 192x256x64 NT bf16': 'PP 192x256 waves 2x4 of 3x2 K=64 colstat=96',
    'forced tile 83 pp 23 192x256x64 NN bf16': 'PP 192x256 waves 2x4 of 3x2 K=64 colstat=96',
    'forced tile 83 pp 23 192x256x64 TN bf16': 'PP 256x256 waves 2x4 of 4x2 K=64 colstat=128',
    'forced tile 83 pp 23 1000x768x320 NT bf16': 'PP 192x256 waves 2x4 of 3x2 K=320 colstat=96',
    'forced tile 83 pp 23 1000x768x320 NN bf16': 'PP 192x256 waves 2x4 of 3x2 K=320 colstat=96',
    'forced tile 83 pp 23 1000x768x320 TN bf16': 'PP 256x256 waves 2x4 of 4x2 K=320 colstat=128',
    'forced tile 84 pp 0 600x520x192 NT bf16': 'BIG 256x256 waves 2x4 of 4x2 K=192 colstat=128',
    'forced tile 84 pp 0 600x520x192 NN bf16': 'BIG 256x256 waves 2x4 of 4x2 K=192 colstat=128',
    'forced tile 84 pp 0 600x520x192 TN bf16': 'BIG 256x256 waves 2x4 of 4x2 K=192 colstat=128',
    'forced tile 84 pp 0 192x256x64 NT bf16': 'BIG 256x256 waves 2x4 of 4x2 K=64 colstat=128',
    'forced tile 84 pp 0 192x256x64 NN bf16': 'BIG 256x256 waves 2x4 of 4x2 K=64 colstat=128',
    'forced tile 84 pp 0 192x256x64 TN bf16': 'BIG 256x256 waves 2x4 of 4x2 K=64 colstat=128',
    'forced tile 84 pp 0 1000x768x320 NT bf16': 'BIG 256x256 waves 2x4 of 4x2 K=320 colstat=128',
    'forced tile 84 pp 0 1000x768x320 NN bf16': 'BIG 256x256 waves 2x4 of 4x2 K=320 colstat=128',
    'forced tile 84 pp 0 1000x768x320 TN bf16': 'BIG 256x256 waves 2x4 of 4x2 K=320 colstat=128',
    'forced tile 84 pp 23 600x520x192 NT bf16': 'PP 256x256 waves 2x4 of 4x2 K=192 colstat=128',
    'forced tile 84 pp 23 600x520x192 NN bf16': 'PP 256x256 waves 2x4 of 4x2 K=192 colstat=128',
    'forced tile 84 pp 23 600x520x192 TN bf16': 'PP 256x256 waves 2x4 of 4x2 K=192 colstat=128',
    'forced tile 84 pp 23 192x256x64 NT bf16': 'PP 256x256 waves 2x4 of 4x2 K=64 colstat=128',
    'forced tile 84 pp 23 192x256x64 NN bf16': 'PP 256x256 waves 2x4 of 4x2 K=64 colstat=128',
    'forced tile 84 pp 23 192x256x64 TN bf16': 'PP 256x256 waves 2x4 of 4x2 K=64 colstat=128',
    'forced tile 84 pp 23 1000x768x320 NT bf16': 'PP 256x256 waves 2x4 of 4x2 K=320 colstat=128',
    'forced tile 84 pp 23 1000x768x320 NN bf16': 'PP 256x256 waves 2x4 of 4x2 K=320 colstat=128',
    'forced tile 84 pp 23 1000x768x320 TN bf16': 'PP 256x256 waves 2x4 of 4x2 K=320 colstat=128',
    'forced mixed 1100x520x1024 NT bf16': 'MIXED 256x256 waves 2x4 of 4x2 K=1024 rows=1+5 colstat=32',
    'forced mixed 1100x520x1024 NN bf16': 'MIXED 256x256 waves 2x4 of 4x2 K=1024 rows=1+5 colstat=32',
    'forced split tile 11 264x264x1100 TN bf16': 'RING 64x64 waves 2x2 of 1x1 K=1152 splits=4x320 +reduce colstat=0',
    'forced split tile 11 200x264x1024 NN bf16': 'RING 64x64 waves 2x2 of 1x1 K=1024 splits=4x256 +reduce colstat=0',
    'forced split tile 11 1032x1032x1100 TN bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=1152 splits=2x576 +reduce colstat=0',
    'forced split tile 11 800x872x1024 NN bf16': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=1024 splits=3x384 +reduce colstat=0',
    'forced split tile 12 264x264x1100 TN bf16': 'RING 64x128 waves 2x2 of 1x2 K=1152 splits=4x320 +reduce colstat=0',
    'forced split tile 12 200x264x1024 NN bf16': 'RING 64x128 waves 2x2 of 1x2 K=1024 splits=4x256 +reduce colstat=0',
    'forced split tile 12 1032x1032x1100 TN bf16': 'LDS_DMA 64x128 waves 1x2 of 2x2 K=1152 splits=3x384 +reduce colstat=0',
    'forced split tile 12 800x872x1024 NN bf16': 'LDS_DMA 64x128 waves 1x2 of 2x2 K=1024 splits=4x256 +reduce colstat=0',
    'forced split tile 22 264x264x1100 TN bf16': 'RING 128x128 waves 2x2 of 2x2 K=1152 splits=4x320 +reduce colstat=0',
    'forced split tile 22 200x264x1024 NN bf16': 'RING 128x128 waves 2x2 of 2x2 K=1024 splits=4x256 +reduce colstat=0',
    'forced split tile 22 1032x1032x1100 TN bf16': 'LDS_DMA 128x128 waves 2x2 of 2x2 K=1152 splits=4x320 +reduce colstat=0',
    'forced split tile 22 1025x904x1024 NN bf16': 'LDS_DMA 128x128 waves 2x2 of 2x2 K=1024 splits=4x256 +reduce colstat=0',
}
ROUTES_BY_NAME = {
    'PP 4500x2104x2048 NN bf16 acc32': 'BIG 192x256 waves 2x4 of 3x2 K=2048 colstat=96',
    'PP 2900x4104x2048 NN bf16 acc32': 'BIG 256x256 waves 2x4 of 4x2 K=2048 colstat=128',
    'PP 3600x3592x1088 TN bf16 acc32': 'BIG 256x256 waves 2x4 of 4x2 K=1088 colstat=128',
    'big split 200x264x8256 NN bf16 acc32': 'BIG 256x256 waves 2x4 of 4x2 K=8256 splits=26x320 +reduce colstat=0',
    'view ragged N PP 2900x4101x2048 NN bf16 acc32': 'BIG 256x256 waves 2x4 of 4x2 K=2048 colstat=128',
}


def route_of(case):
    return ROUTES_BY_NAME.get(case.name) or ROUTES_BY_PRODUCT[case.name.rsplit(" ", 1)[0]]


def tile_of(case):
    m = re.search(r" (\d+)x(\d+) waves", route_of(case))
    return (int(m.group(1)), int(m.group(2))) if m else (64, 64)         # (SIMPLE: 64 x 64 blocks)


def contract_of(case):
    """Which 16-bit accumulation arithmetic the case's route promises (module docstring)."""
    r = route_of(case)
    return "fp32-once" if (r.startswith("SIMPLE") or "splits=" in r) else "round-add-round"


# ------------------------------------------------------------------ operands
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def int_operand(shape, regime, K, g):
    """Small integers as int8 on the CPU: the regime's operand distribution."""
    if regime == "rounding":
        return torch.randint(-3, 4, shape, generator=g, dtype=torch.int8)
    v = torch.randint(-1, 2, shape, generator=g, dtype=torch.int8)
    if K > 4160:                      # thin the non-zeros to 1/3 per operand: |P| stays exact in bf16 (the builder asserts it)
        v = v * torch.randint(0, 2, shape, generator=g, dtype=torch.int8)
    return v


def poisoned(values, ld, dtype, device, zero_tail=False):
    """values [batch, R, W] (integers) as a view into NaN storage [batch, R + ROW_PAD, ld]; zero_tail: columns W .. ld of the operand's
    own rows hold zeros instead (KPAD_ZERO_TAIL)."""
    b, R, W = values.shape
    assert ld >= W
    store = torch.full((b, R + ROW_PAD, ld), NAN, dtype=dtype, device=device)
    if zero_tail:
        store[:, :R, W:] = 0
    store[:, :R, :W] = values.to(device=device, dtype=dtype)
    return store, store[:, :R, :W]


def poisoned_vec(values, dtype, device):
    store = torch.full((values.numel() + 8,), NAN, dtype=dtype, device=device)
    store[:values.numel()] = values.to(device=device, dtype=dtype)
    return store[:values.numel()]


def default_ld(width, unaligned):
    return width + 5 + (width % 2) if unaligned else ceil_to(width, 8) + 8       # unaligned: always odd


def representable(v, dtype):
    return bool((v.to(torch.float32).to(dtype).double() == v).all()) and bool((v.to(torch.float32).double() == v).all())


def round_to(v, dtype):
    """float64 -> dtype, round to nearest even, ONE rounding (the fp32 step is exact: asserted)."""
    f = v.to(torch.float32)
    assert bool((f.double() == v).all()), "not an exact fp32 value"
    return f.to(dtype).double()


@dataclasses.dataclass
class Built:
    case: Case
    a: torch.Tensor               # operand views as kernels.gemm takes them (2-D, or 3-D batched)
    b: torch.Tensor
    bias: torch.Tensor            # or None
    old: torch.Tensor             # [batch, M, N] float64 integers: the old C (accumulate), else None
    product: torch.Tensor         # [batch, M, N] float64: torch.matmul of the float64 operands
    expected: torch.Tensor        # [batch, M, N] float64
    device: str
    a_store: torch.Tensor = None  # the NaN storages [batch, R + ROW_PAD, ld] behind a and b
    b_store: torch.Tensor = None


@functools.lru_cache(maxsize=3)
def _operands(M, N, K, layout, nbatch, regime, dtype, lda, ldb, unaligned, kpad, device):
    """(A storage, A view, B storage, B view, float64 product) of a plain (strided-batched) product."""
    ta, tb = layout
    dt = DTYPES[dtype]
    g = _gen(M, N, K, ta, tb, nbatch, regime)
    av = int_operand((nbatch, K, M) if ta else (nbatch, M, K), regime, K, g)
    bv = int_operand((nbatch, N, K) if tb else (nbatch, K, N), regime, K, g)
    a_store, a = poisoned(av, lda or default_ld(av.shape[2], unaligned), dt, device, zero_tail=kpad)
    b_store, b = poisoned(bv, ldb or default_ld(bv.shape[2], unaligned), dt, device)
    a64, b64 = a.double(), b.double()
    P = torch.matmul(a64.transpose(1, 2) if ta else a64, b64.transpose(1, 2) if tb else b64)
    return a_store, a, b_store, b, P


def accumulated(x, old, odt, contract):
    """x + old in the output type under the route's accumulation contract (module docstring); an fp32 output is added in fp32 everywhere."""
    if odt == torch.float32 or contract == "fp32-once":
        return round_to(x + old, odt)
    assert contract == "round-add-round"
    return round_to(round_to(x, odt) + old, odt)


def expected_of(case, P, bias, old):
    """The expected [batch, M, N] float64 output and the regime's precondition, from the float64 product alone."""
    odt = case.out_dtype
    x = P
    if bias is not None:
        x = x + (bias.double()[None, :, None] if case.bias == "row" else bias.double()[None, None, :])
    x = x * case.alpha
    if case.regime == "exact":
        steps = [P, x] + ([x + old] if old is not None else [])
        for i, s in enumerate(steps):
            assert representable(s, odt), (case.name, f"exact regime: step {i} is not representable in {odt}", float(s.abs().max()))
        return steps[-1]
    assert case.regime == "rounding" and 9 * case.K < 2 ** 24 and float(P.abs().max()) < 2 ** 24, case.name
    return round_to(x, odt) if old is None else accumulated(x, old, odt, contract_of(case))


def build(case, device="cpu"):
    assert case.regime in ("exact", "rounding") and case.alpha in (1.0, 0.5, -2.0) and plan_twin_ok(case), case.name
    assert not (case.regime == "rounding" and case.accumulate and case.bias), case.name
    if case.heads:
        return _build_heads(case, device)
    dt = DTYPES[case.dtype]
    a_store, a, b_store, b, P = _operands(case.M, case.N, case.K, case.layout, case.batch, case.regime, case.dtype, case.lda, case.ldb,
                                          case.unaligned, case.a_kpad_zero, device)
    g = _gen(case.name)
    bias = None
    if case.bias:
        bias = poisoned_vec(torch.randint(-3, 4, (case.M if case.bias == "row" else case.N,), generator=g), dt, device)
    old = torch.randint(-3, 4, (case.batch, case.M, case.N), generator=g).to(device).double() if case.accumulate else None
    exp = expected_of(case, P, bias, old)
    if case.batch == 1:
        a, b = a[0], b[0]
    return Built(case, a, b, bias, old, P, exp, device, a_store, b_store)


def new_output(bt):
    """(storage [batch, M + ROW_PAD, ldc] of NaN, the [batch, M, N] view the call writes): prefilled with the old integers inside
    [M, N] for accumulation."""
    c = bt.case
    ldc = c.ldc or c.N4 + 8
    assert ldc > c.N4 or set(c.exceptions) & {FOLD_DENSE_OUT, HEADS_S_PAD}, c.name
    store = torch.full((c.nbatch, c.M + ROW_PAD, ldc), NAN, dtype=c.out_dtype, device=bt.device)
    out = store[:, :c.M, :c.N]
    if bt.old is not None:
        out.copy_(bt.old)
    return store, out


# ------------------------------------------------------------------ kernels.gemm_heads: operands on [B, T, heads * hd] rows
HD = 64


def _packed(values, device, dt):
    """values [B, heads, rows, HD] -> storage [B, rows + ROW_PAD, heads * HD + 8] of NaN; product (b, h) starts at b * s2 + h * HD."""
    B, Hh, rows, hd = values.shape
    store = torch.full((B, rows + ROW_PAD, Hh * hd + 8), NAN, dtype=dt, device=device)
    store[:, :rows, :Hh * hd] = values.permute(0, 2, 1, 3).reshape(B, rows, Hh * hd).to(device=device, dtype=dt)
    return store, dict(ld=store.stride(1), s=hd, s2=store.stride(0))


def _stacked(values, ld, device, dt):
    """values [B, heads, rows, cols] -> storage [B * heads, rows + ROW_PAD, ld] of NaN; product (b, h) starts at (b * heads + h) * s."""
    B, Hh, rows, cols = values.shape
    store, _ = poisoned(values.reshape(B * Hh, rows, cols), ld, dt, device)
    return store, dict(ld=ld, s=store.stride(0), s2=Hh * store.stride(0))


def _build_heads(case, device):
    B, Hh, product = case.heads
    dt = DTYPES[case.dtype]
    M, N, K = case.M, case.N, case.K
    g = _gen(case.name)
    if product == "scores":          # NT: q [B, T, D] x k [B, S, D] -> [B heads, T, S padded]
        av, bv = int_operand((B, Hh, M, K), case.regime, K, g), int_operand((B, Hh, N, K), case.regime, K, g)
        (a_store, ga), (b_store, gb) = _packed(av, device, dt), _packed(bv, device, dt)
        P = torch.matmul(av.to(device).double(), bv.to(device).double().transpose(2, 3))
    elif product == "context":       # NN: p [B heads, T, S padded] x v [B, S, D] -> [B, T, D]
        av, bv = int_operand((B, Hh, M, K), case.regime, K, g), int_operand((B, Hh, K, N), case.regime, K, g)
        (a_store, ga), (b_store, gb) = _stacked(av, case.lda, device, dt), _packed(bv, device, dt)
        P = torch.matmul(av.to(device).double(), bv.to(device).double())
    else:                            # dvalue, TN: p^T [B heads, T, S padded] x do [B, T, D] -> [B, S, D]
        av, bv = int_operand((B, Hh, K, M), case.regime, K, g), int_operand((B, Hh, K, N), case.regime, K, g)
        (a_store, ga), (b_store, gb) = _stacked(av, case.lda, device, dt), _packed(bv, device, dt)
        P = torch.matmul(av.to(device).double().transpose(2, 3), bv.to(device).double())
    P = P.reshape(B * Hh, M, N)
    old = torch.randint(-3, 4, (B * Hh, M, N), generator=g).to(device).double() if case.accumulate else None
    bt = Built(case, a_store, b_store, None, old, P, expected_of(case, P, None, old), device, a_store, b_store)
    bt.geom = (ga, gb)
    return bt


def heads_output(bt):
    """(storage, geometry, expected storage, unspecified mask) of a gemm_heads product's output."""
    c = bt.case
    B, Hh, product = c.heads
    exp = bt.expected.reshape(B, Hh, c.M, c.N)
    if product == "scores":
        store, geom = _stacked(torch.zeros(B, Hh, c.M, c.N), c.ldc, bt.device, c.out_dtype)
        view = store[:, :c.M, :c.N]
        want = torch.full(store.shape, NAN, dtype=torch.float64, device=bt.device)
        want[:, :c.M, :c.N] = bt.expected
        skip = torch.zeros(store.shape, dtype=torch.bool, device=bt.device)
        skip[:, :c.M, c.N:c.N4] = True
    else:
        store, geom = _packed(torch.zeros(B, Hh, c.M, c.N), bt.device, c.out_dtype)
        view = store[:, :c.M, :Hh * c.N].view(B, c.M, Hh, c.N).permute(0, 2, 1, 3)         # [B, heads, M, N]
        want = torch.full(store.shape, NAN, dtype=torch.float64, device=bt.device)
        want[:, :c.M, :Hh * c.N] = exp.permute(0, 2, 1, 3).reshape(B, c.M, Hh * c.N)
        skip = torch.zeros(store.shape, dtype=torch.bool, device=bt.device)
    view.fill_(NAN)
    if bt.old is not None:
        view.copy_(bt.old.reshape(B, Hh, c.M, c.N))
    return store, geom, want, skip


# ------------------------------------------------------------------ the grouped launch (kernels.gemm_group_tn)
GROUP = [(264, 200, 136), (768, 768, 40), (264, 256, 1088), (256, 1024, 1568)]       # (m, n, k) of out[m, n] += alpha dy[k, m]^T x[k, n]
GROUP_ALPHA = (1.0, 0.5, -2.0, 1.0)
GROUP_SPLITS = [1, 1, 5, 7]        # ofa_gemm_group_plan (host only, pinned on the CPU): one K-slice reaches a 16-bit out in the kernel's
#                                    epilogue (the direct path, round-add-round), a split product goes through fp32 slabs and the fold


# ------------------------------------------------------------------ column statistics (kernels.gemm_colstat)
# (M, N, K, column bias, route): the two products land on different epilogues -- a wave's 64 rows per partial row, and the ring's 32
COLSTAT = [(784, 256, 256, False, "RING 64x64 waves 2x2 of 1x1 K=256 colstat=32"), (200, 136, 72, True, "REG 64x64 waves 1x1 of 2x2 K=72 colstat=64")]


# ------------------------------------------------------------------ the checker
def expected_storage(case, expected, storage_shape, device):
    """(what the whole output storage must hold -- the expected value inside [M, N], NaN outside --, the unspecified region [N, N4))."""
    want = torch.full(storage_shape, NAN, dtype=torch.float64, device=device)
    want[:, :case.M, :case.N] = expected
    skip = torch.zeros(storage_shape, dtype=torch.bool, device=device)
    skip[:, :case.M, case.N:case.N4] = True
    return want, skip


def compare(got, want, skip, tile=(64, 64), what=""):
    """Per element of the whole storage [batch, rows, ld]: where `want` is finite the output is finite and == it; where `want` is NaN
    the output is still NaN; `skip` is not compared.  Raises AssertionError naming the wrong elements and their tile coordinates."""
    assert got.shape == want.shape == skip.shape, (what, got.shape, want.shape)
    g = got.double()
    inside = torch.isfinite(want)
    bad = torch.where(inside, ~(torch.isfinite(g) & (g == want)), ~torch.isnan(g)) & ~skip
    nbad = int(bad.sum())
    if nbad == 0:
        return
    bm, bn = tile
    lines = []
    for z, m, n in bad.nonzero()[:8].tolist():
        where = "inside" if bool(inside[z, m, n]) else "outside [M, N]: must stay NaN"
        lines.append(f"  [{z}, {m}, {n}] got {float(g[z, m, n])} want {float(want[z, m, n])} ({where}): tile ({m // bm}, {n // bn}) of {bm}x{bn}, "
                     f"sub-tile ({m % bm // 32}, {n % bn // 32}), m % 32 = {m % 32}, n % 8 = {n % 8}")
    raise AssertionError(f"{what}: {nbad} wrong elements of {bad.numel()}; the first:\n" + "\n".join(lines))


def check(case, storage, expected):
    want, skip = expected_storage(case, expected, storage.shape, storage.device)
    compare(storage, want, skip, tile_of(case), f"{case.name} [{route_of(case)}]")


# ------------------------------------------------------------------ running a case through the library (GPU)
def run_case(K, case, device="cuda", reps=2):
    """The case through kernels.gemm / kernels.gemm_heads, `reps` times into fresh NaN outputs, every element checked."""
    bt = build(case, device)
    for _ in range(reps):
        if case.heads:
            _run_heads(K, bt)
            continue
        store, out = new_output(bt)
        q = K.FoldQueue() if case.fold else None
        K.gemm(bt.a, bt.b, bool(case.layout[0]), bool(case.layout[1]), bias=bt.bias, bias_row=case.bias == "row", alpha=case.alpha,
               out=out if case.batch > 1 else out[0], accumulate=case.accumulate, out_f32=case.out_f32, a_kpad_zero=case.a_kpad_zero, fold=q)
        if q is not None:
            assert len(q.jobs) == 1, (case.name, "the split-K reduce was not deferred to the fold")
            q.flush()
        check(case, store, bt.expected)


def _run_heads(K, bt):
    c = bt.case
    B, Hh, _ = c.heads
    store, gc, want, skip = heads_output(bt)
    ga, gb = bt.geom
    K.gemm_heads(bt.a, bt.b, store, c.M, c.N, c.K, bool(c.layout[0]), bool(c.layout[1]), ga["ld"], gb["ld"], gc["ld"], B, Hh,
                 ga["s"], ga["s2"], gb["s"], gb["s2"], gc["s"], gc["s2"], alpha=c.alpha, accumulate=c.accumulate)
    compare(store, want, skip, tile_of(c), f"{c.name} [{route_of(c)}]")


def set_env(case):
    """Planner overrides of the debug library for a forced case (read on every call, OFA_GEMM_SPLIT_MIN_K once per process)."""
    import os
    for k in ("OFA_GEMM_TILE", "OFA_GEMM_PP", "OFA_GEMM_MIXED"):
        os.environ.pop(k, None)
    for k, v in case.env:
        if k == "OFA_GEMM_SPLIT_MIN_K":
            assert os.environ.get(k) == v, "OFA_GEMM_SPLIT_MIN_K is read once: it is set by the parent process"
        elif v != "0" or k != "OFA_GEMM_TILE":
            os.environ[k] = v


def forced_groups():
    """Forced cases by subprocess: OFA_GEMM_SPLIT_MIN_K is read once, so its cases get a process of their own."""
    groups = {}
    for c in CASES.values():
        if c.env:
            e = dict(c.env)
            key = "split" if "OFA_GEMM_SPLIT_MIN_K" in e else "mixed" if "OFA_GEMM_MIXED" in e else "big" if "OFA_GEMM_PP" in e else "small"
            groups.setdefault(key, []).append(c.name)
    return groups


OVERRIDES = ("OFA_GEMM_TILE", "OFA_GEMM_PP", "OFA_GEMM_MIXED", "OFA_GEMM_SPLIT_MIN_K")


def run_child(mode, group, timeout=300):
    """main(mode, group) in a fresh process that loads the debug library (planner overrides compiled in): the CompletedProcess.  A child
    that outlives `timeout` raises; nothing is retried."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dbg = os.path.join(root, "ofasys_amd", "libofasys_amd_dbg.so")
    assert os.path.exists(dbg), "the debug library (planner overrides compiled in) is not built: make -C ofasys_amd/csrc debug"
    env = {k: v for k, v in os.environ.items() if k not in OVERRIDES}
    env["OFASYS_AMD_LIB"] = dbg
    if group == "split":
        env["OFA_GEMM_SPLIT_MIN_K"] = "256"
    code = "import sys; sys.path.insert(0, sys.argv[1]); from tests import gemm_exact as G; G.main(sys.argv[2:])"
    return subprocess.run([sys.executable, "-c", code, root, mode, group], env=env, capture_output=True, text=True, timeout=timeout)


def main(argv):
    """Subprocess entry (debug library in OFASYS_AMD_LIB): `plan <group>` prints the route of every forced case of the group, one JSON
    line (host only); `run <group>` runs them on the GPU and prints `forced ok <n>`."""
    import json
    mode, group = argv
    names = forced_groups()[group]
    if mode == "plan":
        from tests.test_gemm_plan_cpu import describe, plan
        out = {}
        for n in names:
            set_env(CASES[n])
            out[n] = describe(plan(*CASES[n].plan_args()))
        print("ROUTES " + json.dumps(out))
        return
    from ofasys_amd import kernels
    for n in names:
        set_env(CASES[n])
        run_case(kernels, CASES[n])
    torch.cuda.synchronize()
    print("forced ok", len(names))


if __name__ == "__main__":
    import sys
    main(sys.argv[1:])
