"""A plain-torch / numpy oracle for the streaming kernels of csrc/elementwise.hip and the step tail of csrc/loss_optim.hip: no GPU needed,
no dependency on the kernels.  It follows tests/rownorm_oracle.py and takes excess(), grad_excess(), floor_of(), EPS, NVEC and the GELU
magnitude helpers from there.

Grids, restated: grid_for() (every streaming kernel: ceil(work / 256) blocks, at most 2048 = 524 288 threads, one 16-byte vector each),
sumsq_grid() (at most 1024 blocks) and adam_grid() (one thread per parameter, at most 65 536 blocks or the test's max_blocks; a thread
takes the quads q0 and q0 + stride of a trip).  Every case is named by where it sits against its grid:
  below   one vector, N - 1 elements (tail only, where the kernel has a tail), 255 and 257 vectors
  at      exactly `threads` vectors: the full grid on its one trip
  past    threads + 300 vectors (+ a tail of N - 3 elements): blocks 0 and 1 make a second trip, block 1 on 44 threads only
and the row-shaped kernels get `past` twice: D = N (one vector per row, 524 588 rows) and 96 vectors per row (768 columns in 16 bits,
384 in fp32; 5465 rows, row 5461 straddles the trip seam).

Three kinds of check:
  movers            embedding_fwd, gather_rows, gather_rows_parts, scatter_rows_part, im2col_patch and the dropout mask: bit for bit
                    against index arithmetic in torch (*_expected) and a Philox4x32-10 restatement in integer numpy (dropout_mask)
  one rounding      GELU forward / backward, dropout + residual, add_rowvec_mask, mul, scale_row_groups, add_n, batch_sum:
                    *_reference() in float64 on the stored inputs with the componentwise magnitude bound (0: exactly 0), *_emulate() in
                    float32 with the kernel's rounding points and nothing else of it, taking one named mutation
  exact reductions  sumsq, sumsq_schedule, colsum, reduce_sum_f32 on integers in [-2, 2]: every partial sum stays below 2^24, so any
                    summation order gives the same fp32 and the integer sum is the only answer; one randn case each against float64
                    within c 2^-24 sum|terms|, c counted along the longest chain of additions (SUMSQ_CHAIN, COLSUM_CHAIN)
and Adam: adam_reference() in float64 with every scalar taken as the fp32 value the kernel receives, adam_emulate() with its mutations.
tests/test_stream_oracle_cpu.py proves the tables sound; tests/test_stream_edges_gpu.py runs them against the kernels."""
import math
from collections import namedtuple

import numpy as np
import torch

from tests.rownorm_oracle import (BF16, DTYPES3, EPS, F32, F64, FP16, INV_SQRT2, INV_SQRT_2PI, NAMES, NVEC, PLANT, _gelu, _gelu_abs,  # noqa: F401
                                  _gpa, cdiv, excess, floor_of, grad_excess)

# ---------------------------------------------------------------------------------------------------------------- measured constants
# CEILING: the cap on excess(emulate, reference, bound) of the 16-bit outputs over the whole table: one rounding of the result.
# Measured 2026-10-21 (tests/test_stream_oracle_cpu.py prints the figures with -s), the emulation's worst excess in eps:
#          gelu_fwd  gelu_bwd  dropout_add  add_rowvec_mask  mul    scale_row_groups  add_n  batch_sum
#   bf16   0.967     0.996     0.996        0.996            0.988  0.996             0.996  0.996
#   fp16   0.980     0.999     0.999        0.999            0.999  0.999             0.999  0.999
CEILING = 1.0
# TOL for the kernels = 2 * CEILING: the factor covers device erff / __expf / v_rcp_f32 against host libm.  Never set from a kernel.
TOL = 2.0 * CEILING
# fp32 outputs (fp32 tensors; Adam's m, v and master in every dtype): error / bound, 8 x the emulation's worst against float64.
# Measured 2026-10-21, the emulation's worst over the tables:
#   gelu_fwd 1.31e-7, gelu_bwd 1.78e-7, dropout_add 1.60e-7, add_rowvec_mask 1.15e-7, mul 5.96e-8, scale_row_groups 5.96e-8,
#   add_n 1.02e-7, batch_sum 1.10e-7;  Adam (worst of the three gradient dtypes): m 1.42e-7, v 2.28e-7, master 2.90e-7
G32 = {"gelu_fwd": 8 * 1.4e-7, "gelu_bwd": 8 * 1.8e-7, "dropout_add": 8 * 1.7e-7, "add_rowvec_mask": 8 * 1.2e-7, "mul": 8 * 6.0e-8,
       "scale_row_groups": 8 * 6.0e-8, "add_n": 8 * 1.1e-7, "batch_sum": 8 * 1.2e-7,
       "adam": {"m": 8 * 1.5e-7, "v": 8 * 2.3e-7, "p": 8 * 3.0e-7}}
# The kernels themselves on an MI355X, worst over the same tables (tests/test_stream_edges_gpu.py prints them with -s):
#   2026-10-21, 16-bit outputs, excess in eps against TOL = 2.0:
#          gelu_fwd  gelu_bwd  dropout_add  add_rowvec_mask  mul    scale_row_groups  add_n  batch_sum
#   bf16   0.967     0.996     0.996        0.996            0.988  0.996             0.996  0.996
#   fp16   0.980     0.999     0.999        0.999            0.999  0.999             0.999  0.999
#   fp32 outputs, error / bound, of 8 x the emulation's figure above: gelu_fwd 1.44e-7, gelu_bwd 1.74e-7, dropout_add 1.60e-7,
#   add_rowvec_mask 1.15e-7, mul 5.96e-8, scale_row_groups 5.96e-8, add_n 1.02e-7, batch_sum 1.10e-7;
#   Adam: m 1.42e-7, v 2.28e-7, master 1.21e-7 (the second quad ran on 10, 256 and 512 threads, the second trip on 10 and 512 + 100 quads)
#   movers, the dropout mask, the model copy, capped against default grid, the skipped update: every bit; sumsq, colsum and
#   reduce_sum_f32 on integers: exact; on randn at most 0.034 (sumsq) and 0.003 (colsum) of the chain bounds.  No fault found.

STREAM_CAP, SUMSQ_CAP, ADAM_CAP = 2048, 1024, 65536
STREAM_T, SUMSQ_T = STREAM_CAP * 256, SUMSQ_CAP * 256               # threads = vectors per trip of a capped grid
WIDE = 96                                                             # vectors per row of the wide row shape: 768 / 384 columns
SEED, SENTINEL = 1234, 0xAB


# ---------------------------------------------------------------------------------------------------------------- grids, restated
def grid_for(work):
    return min(max(cdiv(work, 256), 1), STREAM_CAP)


def sumsq_grid(n, dtype):
    return min(max(cdiv(n // NVEC[dtype], 256), 1), SUMSQ_CAP)


def adam_grid(n, max_blocks=0):
    return min(cdiv(n, 256), max_blocks if max_blocks > 0 else ADAM_CAP)


def where(work, threads):
    """below / at / past: `work` grid-stride items against the threads of the launched grid."""
    return "below" if work < threads else ("at" if work == threads else "past")


def adam_trips(n, max_blocks=0):
    """-> (threads that own a second quad in the first trip, quads of the second trip, second quads of the second trip)."""
    stride, nq = adam_grid(n, max_blocks) * 256, n >> 2
    return max(0, min(nq, 2 * stride) - stride), max(0, min(nq, 3 * stride) - 2 * stride), max(0, min(nq, 4 * stride) - 3 * stride)


# ---------------------------------------------------------------------------------------------------------------- Philox4x32-10
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints), key: two ints -> four uint32 arrays: common.h's round function in uint64 numpy."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) for x in ctr]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


PHILOX_KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
              ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox_thresh(p):
    """(uint32)(p * 65536.0f + 0.5f): round(p 65536) in fp32."""
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def dropout_mask(n, p, seed, offset, mutation=None, threads=STREAM_T):
    """bool [n]: element e is kept iff halfword e % 8 of Philox(counter = offset + e / 8, key = seed) >= round(p 65536)."""
    nq = cdiv(n, 8)
    q = np.arange(nq, dtype=np.uint64)
    if mutation == "philox_counter_is_thread_index":
        q = q % np.uint64(threads)
    ctr = np.uint64(offset % (1 << 64)) + q                                    # (wraps mod 2^64 as the kernel's uint64 does)
    r = philox4x32_10((ctr & MASK32, ctr >> np.uint64(32), 0, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    hw = np.empty((nq, 8), dtype=np.uint32)
    for j in range(8):
        jj = j ^ 1 if mutation == "mask_halfword_swapped" else j
        w = r[j >> 1]
        hw[:, jj] = (w >> np.uint32(16)) if j & 1 else (w & np.uint32(0xFFFF))
    return torch.from_numpy((hw >= philox_thresh(p)).reshape(-1)[:n].copy())


# ---------------------------------------------------------------------------------------------------------------- cases
# units: vectors (flat kernels, vpr == 0) or rows (row-shaped kernels, vpr = vectors per row); tail k > 0: N - k more elements
Case = namedtuple("Case", "name kernel pos units vpr tail regime opt seed")
ONE_ROUNDING = ("gelu_fwd", "gelu_bwd", "dropout_add", "add_rowvec_mask", "mul", "scale_row_groups", "add_n", "batch_sum")
MOVERS = ("embedding_fwd", "gather_rows", "gather_rows_parts", "scatter_rows_part", "im2col_patch")
HAS_TAIL = ("gelu_fwd", "gelu_bwd", "dropout_add", "add_n")
ROW_SHAPED = ("add_rowvec_mask", "mul", "scale_row_groups", "embedding_fwd", "gather_rows", "gather_rows_parts", "scatter_rows_part")
GRID_MUTATIONS = ("second_trip_reads_first_trip", "drop_tail", "drop_last_vector")
MUTATIONS = {"gelu_fwd": GRID_MUTATIONS, "gelu_bwd": GRID_MUTATIONS,
             "dropout_add": GRID_MUTATIONS[:1] + ("philox_counter_is_thread_index", "mask_halfword_swapped", "keep_scale_missing"),
             "add_rowvec_mask": GRID_MUTATIONS[:1] + GRID_MUTATIONS[2:] + ("b_period_ignored",),
             "mul": GRID_MUTATIONS[:1] + GRID_MUTATIONS[2:], "scale_row_groups": GRID_MUTATIONS[:1] + GRID_MUTATIONS[2:] + ("group_off_by_one",),
             "add_n": GRID_MUTATIONS + ("add_n_drops_last_input",), "batch_sum": GRID_MUTATIONS[:1] + GRID_MUTATIONS[2:] + ("batch_sum_overwrites",)}
MOVER_MUTATIONS = ("second_trip_reads_first_trip", "drop_last_vector")
MASK_MUTATIONS = ("philox_counter_is_thread_index", "mask_halfword_swapped")
GELU_POINTS = (0.0, -0.0, 1e-4, -1e-4, 5.0, -5.0, 9.0, -9.0, 40.0, -40.0)


def vec_n(case, dtype):
    """Elements per grid-stride item: a 16-byte vector; dropout walks quads of 8 elements in every dtype; the scalar routes one."""
    if case.kernel == "dropout_add":
        return 8
    if case.kernel == "embedding_fwd" and case_D(case, dtype) % NVEC[dtype]:
        return 1
    if case.kernel == "im2col_patch":
        return 8 if im2col_runs(case, dtype) else 1
    return NVEC[dtype]


def case_D(case, dtype):
    return dict(case.opt).get("D") or case.vpr * NVEC[dtype]


def case_numel(case, dtype):
    """Elements of the output."""
    if case.kernel == "im2col_patch":
        o = dict(case.opt)
        return o["B"] * (o["lead"] + (o["H"] // o["p"]) * (o["W"] // o["p"])) * o["Kpad"]
    if case.vpr or dict(case.opt).get("D"):
        return case.units * case_D(case, dtype)
    N = vec_n(case, dtype)
    return case.units * N + (N - case.tail if case.tail else 0)


def case_work(case, dtype):
    """Items the grid-stride loop walks (whole vectors; the dropout kernel's last quad may be partial)."""
    n, N = case_numel(case, dtype), vec_n(case, dtype)
    return cdiv(n, N) if case.kernel == "dropout_add" else n // N


def case_grid(case, dtype):
    w = case_work(case, dtype)
    return grid_for(w + 1 if case.kernel == "add_n" else w)


def case_where(case, dtype):
    return where(case_work(case, dtype), case_grid(case, dtype) * 256)


def case_pos(case, dtype):
    """Where the case's name says it sits."""
    return dict(case.opt).get("pos32", case.pos) if dtype == F32 else case.pos


def _flat_sizes(T, tail):
    return ([("below", 1, 0)] + ([("below", 0, 1)] if tail else []) +
            [("below", 255, 0), ("below", 257, 0), ("at", T, 0), ("past", T + 300, 3 if tail else 0)])


def _row_sizes(T):
    return [("below", 1, 1), ("below", 255, 1), ("below", 257, 1), ("at", T, 1), ("past", T + 300, 1), ("past", 5465, WIDE)]


def _cases():
    out, seed = [], [5000]

    def add(kernel, pos, units, vpr, tail, regime, **opt):
        what = " ".join(f"{k}={v}" for k, v in opt.items())
        shape = f"rows{units} vpr{vpr}" if vpr else f"vec{units}" + (f" tail-{tail}" if tail else "")
        out.append(Case(f"{kernel} {pos} {shape} {regime} {what}".strip(), kernel, pos, units, vpr, tail, regime, tuple(opt.items()), seed[0]))
        seed[0] += 1

    def regime(pos, i):
        return "planted" if pos == "past" and i % 2 == 0 or pos == "below" and i % 2 else "randn"

    for kernel in ("gelu_fwd", "gelu_bwd"):
        for i, (pos, u, t) in enumerate(_flat_sizes(STREAM_T, True)):
            add(kernel, pos, u, 0, t, "planted" if pos == "past" else ("randn", "planted")[i % 2])
    # dropout: offsets 0 and 77, offset_base on the device, a low word that wraps during the launch; p 0, 0.1, 0.5; with and without residual
    drops = ((0.1, 0, 0, True), (0.5, 77, 0, False), (0.0, 77, 0, True), (0.1, 77, 12345, True), (0.1, 2 ** 32 - 1000, 0, True),
             (0.5, 0, 2 ** 32 - 77 - 1000, True))
    for i, (pos, u, t) in enumerate(_flat_sizes(STREAM_T, True)):
        p, off, base, res = drops[i % len(drops)]
        add("dropout_add", pos, u, 0, t, "planted" if pos == "past" else "randn", p=p, offset=off, base=base, res=res)
    add("dropout_add", "past", STREAM_T + 300, 0, 3, "randn", p=0.1, offset=2 ** 32 - 1000, base=0, res=False)
    add("dropout_add", "past", STREAM_T + 300, 0, 3, "randn", p=0.5, offset=0, base=77, res=True)
    add("dropout_add", "below", 257, 0, 0, "randn", p=0.0, offset=0, base=0, res=False)
    for i, (pos, u, vpr) in enumerate(_row_sizes(STREAM_T)):
        # b_period 0 and 7 (7 divides neither 524 288 vectors nor the 5461.33 rows of a wide trip); vec on and off; a masked row at the seam
        add("add_rowvec_mask", pos, u, vpr, 0, regime(pos, i), period=(0, 7)[i % 2] if u > 7 else 0, b=i != 2, vec=i % 3 != 1, mask=i != 0)
        add("mul", pos, u, vpr, 0, regime(pos, i), rowvec=i % 2)
        # a group boundary at the seam: D = N, 4 rows per group (524 288 = 4 * 131 072); wide rows, 5461 per group: row 5461 straddles it
        add("scale_row_groups", pos, u, vpr, 0, regime(pos, i), group=5461 if vpr == WIDE else (4 if u > 4 else 1))
    add("add_rowvec_mask", "past", 5465, WIDE, 0, "randn", period=0, b=True, vec=False, mask=True)
    add("mul", "past", 5465, WIDE, 0, "planted", rowvec=1)
    for i, (pos, u, t) in enumerate(_flat_sizes(STREAM_T, True)):       # 1, 2 and 16 inputs; the 16 at the small sizes
        add("add_n", pos, u, 0, t, "planted" if pos == "past" else "randn", k=(16, 2, 1, 16, 1, 2)[i])
    for i, (pos, u, t) in enumerate(_flat_sizes(STREAM_T, False)):      # batch 1 and 5, accumulate on and off
        add("batch_sum", pos, u, 0, 0, "planted" if pos == "past" else "randn", batch=(5, 1, 5, 1, 1)[i], acc=(0, 1, 1, 0, 1)[i])
    add("batch_sum", "below", 257, 0, 0, "randn", batch=1, acc=0)
    # ---- movers
    for i, (pos, u, vpr) in enumerate(_row_sizes(STREAM_T)):
        add("embedding_fwd", pos, u, vpr, 0, "ids", pad=i % 2)
        add("gather_rows", pos, u, vpr, 0, "ids")
        add("gather_rows_parts", pos, u, vpr, 0, "ids", parts=(1, 3, 8)[i % 3])
        add("scatter_rows_part", pos, u, vpr, 0, "ids")
    for D in (12, 13):                                                   # the scalar route (fp32 takes D = 12 as three vectors)
        for pos, rows in (("below", 1), ("below", 21), ("past", cdiv(STREAM_T + 300, D))):
            add("embedding_fwd", pos, rows, 0, 0, "ids", D=D, pad=0, **({"pos32": "below"} if D == 12 else {}))
    # im2col: (B, C, H, W, p, Kpad, lead): 16-bit with even p moves dword runs (8 elements per item), fp32 or odd p one element per item
    # (pos names the 16-bit launch; pos32 the fp32 one, which walks 8 times the items where the 16-bit types move runs)
    for pos, pos32, shape in (("below", "below", (1, 3, 4, 6, 2, 16, 0)), ("below", "below", (3, 2, 8, 8, 2, 8, 1)),
                              ("below", "below", (2, 2, 6, 3, 3, 24, 0)), ("below", "below", (1, 1, 5, 5, 5, 32, 1)),
                              ("at", "past", (4, 3, 512, 512, 2, 16, 0)), ("at", "at", (4, 3, 192, 192, 3, 32, 0)),
                              ("past", "past", (2, 3, 726, 726, 2, 16, 1)), ("past", "past", (2, 2, 315, 315, 3, 24, 1))):
        add("im2col_patch", pos, 0, 0, 0, "img", pos32=pos32, **dict(zip(("B", "C", "H", "W", "p", "Kpad", "lead"), shape)))
    return out


def im2col_runs(case, dtype):
    o = dict(case.opt)
    return dtype != F32 and o["p"] % 2 == 0 and o["Kpad"] % 8 == 0


CASES = _cases()


def cases_of(kernel):
    return [c for c in CASES if c.kernel == kernel]


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def plant_positions(n, N, threads):
    """Flat element ranges of the planted regime: the last vector of trip one, the first and the last vector of trip two, the tail."""
    nvec = n // N
    vs = [v for v in (threads - 1, threads, nvec - 1) if 0 <= v < nvec]
    return [(v * N, v * N + N) for v in vs] + ([(nvec * N, n)] if n % N else [])


def _primary(case, dtype, gen, n):
    x = torch.randn(n, generator=gen)
    if case.regime == "planted":
        for lo, hi in plant_positions(n, vec_n(case, dtype), STREAM_T):
            x[lo:hi] = PLANT
    return x


def build(case, dtype, device="cpu"):
    """The stored inputs of one case -> dict of tensors (on `device`) and scalars."""
    gen, n, k, o = _gen(case.seed), case_numel(case, dtype), case.kernel, dict(case.opt)
    N = NVEC[dtype]
    dev = lambda t: t.to(device) if t is not None else None                # noqa: E731
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dtype)              # noqa: E731
    b = dict(n=n)
    if k in ("gelu_fwd", "gelu_bwd"):
        x = _primary(case, dtype, gen, n)
        pts = torch.tensor(GELU_POINTS)
        if n >= len(pts):
            x[:len(pts)] = pts
        else:
            x[:n] = pts.roll(-4)[:n] if case.regime == "planted" else pts[:n]
        b.update(x=x.to(dtype), dy=rnd(n) if k == "gelu_bwd" else None)
    elif k == "dropout_add":
        b.update(x=_primary(case, dtype, gen, n).to(dtype), res=rnd(n) if o["res"] else None, p=o["p"], offset=o["offset"], base=o["base"],
                 mask=dropout_mask(n, o["p"], SEED, o["offset"] + o["base"]))
    elif k in ("add_rowvec_mask", "mul", "scale_row_groups"):
        rows, D = case.units, case_D(case, dtype)
        b.update(rows=rows, D=D, a=_primary(case, dtype, gen, n).to(dtype).view(rows, D))
        seam = min(rows - 1, STREAM_T // case.vpr)                       # the row that holds the first vector of trip two
        if k == "add_rowvec_mask":
            mask = None
            if o["mask"]:
                mask = torch.rand(rows, generator=gen) < 0.2
                mask[seam] = True
                mask[max(seam - 1, 0)] = rows == 1
            b.update(b=rnd(o["period"] or rows, D) if o["b"] else None, vec=rnd(D) if o["vec"] else None, mask=mask, period=o["period"] if o["b"] else 0)
        elif k == "mul":
            b.update(b=rnd(D) if o["rowvec"] else rnd(rows, D), rowvec=o["rowvec"])
        else:
            b.update(scale=torch.randn(cdiv(rows, o["group"]), generator=gen), group=o["group"])
    elif k == "add_n":
        b.update(ins=[_primary(case, dtype, gen, n).to(dtype)] + [rnd(n) for _ in range(o["k"] - 1)])
    elif k == "batch_sum":
        b.update(x=torch.cat([_primary(case, dtype, gen, n).to(dtype)] + [rnd(n) for _ in range(o["batch"] - 1)]).view(o["batch"], n),
                 prev=rnd(n) if o["acc"] else None)
    elif k == "embedding_fwd":
        rows, D, V = case.units, case_D(case, dtype), 37
        ids = torch.randint(-3, V + 3, (rows,), generator=gen)
        ids[0], ids[-1] = (V, -1) if rows > 1 else (V + 2, V + 2)
        b.update(rows=rows, D=D, w=rnd(V, D), ids=ids, pad_id=1 if o["pad"] else None)
    elif k == "gather_rows":
        rows, D, S = case.units, case_D(case, dtype), 41
        idx = torch.randint(-1, S + 2, (rows,), generator=gen)
        idx[0], idx[-1] = -1, S
        idx[min(rows - 1, STREAM_T)] = S + 1
        b.update(rows=rows, D=D, src=rnd(S, D), index=idx)
    elif k == "gather_rows_parts":
        rows, D, B = case.units, case_D(case, dtype), 3
        lens = {1: [5], 3: [4, 1, 6], 8: [1, 2, 3, 1, 2, 1, 3, 2]}[o["parts"]]
        T = sum(lens)
        idx = torch.randint(-1, B * T + 2, (rows,), generator=gen)
        cover = torch.arange(B * T)                                      # every position: both sides of every part seam, in every sample
        m = min(rows, B * T)
        idx[rows - m:] = cover[:m]
        if rows > STREAM_T:
            idx[STREAM_T - m // 2:STREAM_T - m // 2 + m] = cover[:m]     # ... and across the trip seam
        idx[0] = -1 if rows > 1 else T - 1
        if rows > 2:
            idx[1] = B * T
        b.update(rows=rows, D=D, lens=lens, B=B, parts=[rnd(B, ln, D) for ln in lens], index=idx)
    elif k == "scatter_rows_part":
        rows, D, S = case.units, case_D(case, dtype), 29
        B = next(d for d in (5, 4, 3, 2, 1) if rows % d == 0)
        nk, start = rows // B, 3
        T = nk + 5
        inv = torch.randint(-1, S + 1, (B * T,), generator=gen)
        inv[start] = -1 if nk > 1 else 2
        b.update(rows=rows, D=D, B=B, nk=nk, Ttot=T, start=start, src=rnd(S, D), inverse=inv)
    elif k == "im2col_patch":
        b.update(img=rnd(o["B"], o["C"], o["H"], o["W"]), p=o["p"], Kpad=o["Kpad"], lead=o["lead"])
    else:
        raise KeyError(k)
    return {name: (dev(v) if torch.is_tensor(v) else ([dev(t) for t in v] if isinstance(v, list) and v and torch.is_tensor(v[0]) else v))
            for name, v in b.items()}


# ---------------------------------------------------------------------------------------------------------------- movers
def mover_expected(case, b):
    """Index arithmetic in torch -> {output name: tensor}, bit for bit what the kernel must write."""
    k = case.kernel
    if k == "embedding_fwd":
        V = b["w"].shape[0]
        out = {"out": b["w"][b["ids"].clamp(0, V - 1)]}
        if b["pad_id"] is not None and b["D"] % NVEC[b["w"].dtype] == 0:
            out["is_pad"] = (b["ids"] == b["pad_id"]).to(torch.uint8)
        return out
    if k == "gather_rows":
        src, idx = b["src"], b["index"]
        ok = (idx >= 0) & (idx < src.shape[0])
        return {"out": torch.where(ok[:, None], src[idx.clamp(0, src.shape[0] - 1)], torch.zeros((), dtype=src.dtype, device=src.device))}
    if k == "gather_rows_parts":
        cat, idx = torch.cat(b["parts"], dim=1).reshape(-1, b["D"]), b["index"]      # the concatenation the kernel never builds
        ok = (idx >= 0) & (idx < cat.shape[0])
        return {"out": torch.where(ok[:, None], cat[idx.clamp(0, cat.shape[0] - 1)], torch.zeros((), dtype=cat.dtype, device=cat.device))}
    if k == "scatter_rows_part":
        src = b["src"]
        inv = b["inverse"].view(b["B"], b["Ttot"])[:, b["start"]:b["start"] + b["nk"]].reshape(-1)
        ok = (inv >= 0) & (inv < src.shape[0])
        return {"out": torch.where(ok[:, None], src[inv.clamp(0, src.shape[0] - 1)], torch.zeros((), dtype=src.dtype, device=src.device))}
    if k == "im2col_patch":
        img, p = b["img"], b["p"]
        B, C, H, W = img.shape
        nph, npw, K = H // p, W // p, C * p * p
        col = torch.zeros(B, b["lead"] + nph * npw, b["Kpad"], dtype=img.dtype, device=img.device)
        col[:, b["lead"]:, :K] = img.view(B, C, nph, p, npw, p).permute(0, 2, 4, 1, 3, 5).reshape(B, nph * npw, K)
        return {"out": col.view(-1, b["Kpad"])}
    raise KeyError(k)


def same_bits(a, b):
    """Equality of bits (NaN payloads and the sign of zero included)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool(torch.equal(a.contiguous().view(view), b.contiguous().view(view)))


def grid_mutate(flat, N, threads, mutation, fill):
    """A flat output under one of GRID_MUTATIONS: what a wrong grid-stride loop leaves behind (`fill`: what the buffer held before)."""
    out, n = flat.clone(), flat.numel()
    nvec = n // N
    if mutation == "second_trip_reads_first_trip" and nvec > threads:
        out[threads * N:nvec * N] = flat[:(nvec - threads) * N]
    elif mutation == "drop_tail":
        out[nvec * N:] = fill
    elif mutation == "drop_last_vector" and nvec:
        out[(nvec - 1) * N:nvec * N] = fill
    return out


# ---------------------------------------------------------------------------------------------------------------- one rounding
def _rowsel(b, rows, period):
    r = torch.arange(rows, device=b.device)
    return b[r % period] if period else b


def reference(case, b):
    """float64 on the stored inputs -> (ref, bound), both flat [n]."""
    k = case.kernel
    if k == "gelu_fwd":
        h = b["x"].double()
        return h * _gelu(h)[0], h.abs() * _gelu_abs(h)
    if k == "gelu_bwd":
        h, g = b["x"].double(), b["dy"].double()
        Phi, phi = _gelu(h)
        return g * (Phi + h * phi), g.abs() * _gpa(h, Phi, phi, b["x"].dtype)
    if k == "dropout_add":
        x, m = b["x"].double(), b["mask"].to(b["x"].device).double()
        s = 1.0 / (1.0 - float(np.float32(b["p"])))
        res = b["res"].double() if b["res"] is not None else torch.zeros_like(x)
        return m * s * x + res, m * s * x.abs() + res.abs()
    if k == "add_rowvec_mask":
        ref, bd = b["a"].double(), b["a"].double().abs()
        if b["b"] is not None:
            t = _rowsel(b["b"].double(), b["rows"], b["period"])
            ref, bd = ref + t, bd + t.abs()
        if b["vec"] is not None:
            ref, bd = ref + b["vec"].double(), bd + b["vec"].double().abs()
        if b["mask"] is not None:
            keep = (~b["mask"]).double()[:, None]
            ref, bd = ref * keep, bd * keep
        return ref.reshape(-1), bd.reshape(-1)
    if k == "mul":
        r = b["a"].double() * b["b"].double()
        return r.reshape(-1), r.abs().reshape(-1)
    if k == "scale_row_groups":
        s = b["scale"].double()[torch.arange(b["rows"], device=b["a"].device) // b["group"]][:, None]
        r = b["a"].double() * s
        return r.reshape(-1), r.abs().reshape(-1)
    if k == "add_n":
        st = torch.stack([t.double() for t in b["ins"]])
        return st.sum(0), st.abs().sum(0)
    if k == "batch_sum":
        x = b["x"].double()
        p = b["prev"].double() if b["prev"] is not None else torch.zeros_like(x[0])
        return x.sum(0) + p, x.abs().sum(0) + p.abs()
    raise KeyError(k)


def emulate(case, b, dtype, mutation=None):
    """float32 with the kernel's rounding points (one: the store) -> flat [n] of dtype; mutation: one of MUTATIONS[kernel]."""
    k = case.kernel
    assert mutation is None or mutation in MUTATIONS[k], (k, mutation)
    if k == "gelu_fwd":
        h = b["x"].float()
        y = 0.5 * h * (1.0 + torch.erf(h * 0.70710678118654752440))
    elif k == "gelu_bwd":
        h = b["x"].float()
        y = b["dy"].float() * (0.5 * (1.0 + torch.erf(h * 0.70710678118654752440)) + h * 0.39894228040143267794 * torch.exp(-0.5 * h * h))
    elif k == "dropout_add":
        p32 = torch.tensor(b["p"], dtype=F32)
        s = 1.0 if mutation == "keep_scale_missing" else float(torch.tensor(1.0) / (torch.tensor(1.0) - p32))
        m = b["mask"] if mutation not in MASK_MUTATIONS else dropout_mask(b["n"], b["p"], SEED, b["offset"] + b["base"], mutation)
        y = torch.where(m.to(b["x"].device), b["x"].float() * s, torch.zeros((), device=b["x"].device))
        if b["res"] is not None:
            y = y + b["res"].float()
    elif k == "add_rowvec_mask":
        y = b["a"].float()
        if b["b"] is not None:
            if mutation == "b_period_ignored" and b["period"]:
                y = y + b["b"].float()[torch.arange(b["rows"], device=y.device).clamp_max(b["period"] - 1)]
            else:
                y = y + _rowsel(b["b"].float(), b["rows"], b["period"])
        if b["vec"] is not None:
            y = y + b["vec"].float()
        if b["mask"] is not None:
            y = torch.where(b["mask"][:, None], torch.zeros((), device=y.device), y)
    elif k == "mul":
        y = b["a"].float() * b["b"].float()
    elif k == "scale_row_groups":
        r = torch.arange(b["rows"], device=b["a"].device)
        g = ((r + 1) // b["group"]).clamp_max(b["scale"].numel() - 1) if mutation == "group_off_by_one" else r // b["group"]
        y = b["a"].float() * b["scale"][g][:, None]
    elif k == "add_n":
        ins = b["ins"][:-1] if (mutation == "add_n_drops_last_input" and len(b["ins"]) > 1) else b["ins"]
        y = torch.zeros_like(ins[0], dtype=F32)
        for t in ins:
            y = y + t.float()
    elif k == "batch_sum":
        y = b["prev"].float() if (b["prev"] is not None and mutation != "batch_sum_overwrites") else torch.zeros_like(b["x"][0], dtype=F32)
        for t in b["x"]:
            y = y + t.float()
    else:
        raise KeyError(k)
    y = y.reshape(-1).to(dtype)
    if mutation in GRID_MUTATIONS:
        y = grid_mutate(y, vec_n(case, dtype), case_grid(case, dtype) * 256, mutation, float("nan"))
    return y


def figures(case, b, got, dtype):
    """One case's output against its reference -> {name: figure}: y in eps of the bound (fp32: error / bound); drop: 0 iff every dropped
    element carries the residual's bits (0 without one)."""
    ref, bd = reference(case, b)
    fig = {"y": grad_excess(got.reshape(-1), ref, bd, dtype)}
    if case.kernel == "dropout_add":
        dropped = ~b["mask"].to(got.device)
        want = b["res"][dropped] if b["res"] is not None else torch.zeros(int(dropped.sum()), dtype=dtype, device=got.device)
        fig["drop"] = 0.0 if same_bits(got.reshape(-1)[dropped], want) else float("inf")
    return fig


def limit(kernel, name, dtype, is_kernel=True):
    """The largest figure an output may show: the emulation's cap, or (is_kernel) what the GPU test allows a kernel."""
    if name == "drop":
        return 0.0
    if kernel == "adam":
        return G32["adam"][name] / (1 if is_kernel else 8)
    if dtype == F32:
        return G32[kernel] / (1 if is_kernel else 8)
    return TOL if is_kernel else CEILING


# ---------------------------------------------------------------------------------------------------------------- exact reductions
# sumsq, the longest chain of fp32 additions behind one element of the result at the `past` size (two trips, the tail in block 0):
#   a thread adds N products per vector, two vectors, and (block 0) one tail product ......... 2 N + 1   (17 in 16 bits, 9 in fp32)
#   each product is rounded before it is added (or fused: one rounding less) ................. 1
#   wave_sum: 6 steps; the four waves: 3 additions ......................................... 9
#   the final pass: 1024 partials over 256 threads: 4 additions, wave_sum 6, four waves 3 ..... 13
#   onto `out` .............................................................................. 1
def sumsq_chain(dtype):
    return 2 * NVEC[dtype] + 1 + 1 + 9 + 13 + 1


# colsum at 8200 rows: 128 row groups x 8 row lanes = 1024 rows per pass: 9 additions per thread; the 8 row lanes of a block: 8; the
# final pass: 128 groups over 16 lanes: 8 additions, the 16 lanes: 16; alpha: 1; accumulate: 1
COLSUM_CHAIN = 9 + 8 + 8 + 16 + 1 + 1
U32 = 2.0 ** -24
SUMSQ_SIZES = [(pos, u, t) for pos, u, t in _flat_sizes(SUMSQ_T, True)]
COLSUM_ROWS, COLSUM_SLOT_CAP = (8191, 8192, 8193, 8200), 128
REDUCE_N = (1, 255, 257, 70001)


def sumsq_n(units, tail, dtype):
    N = NVEC[dtype]
    return units * N + (N - tail if tail else 0)


def colsum_slots(rows):
    return min(max(cdiv(rows, 64), 1), COLSUM_SLOT_CAP)


def colsum_passes(rows):
    """Trips of the strided row loop: 8 row lanes per group."""
    return cdiv(rows, colsum_slots(rows) * 8)


def small_ints(n, seed, dtype):
    """Integers in [-2, 2], exact in every dtype."""
    return torch.randint(-2, 3, (n,), generator=_gen(seed)).to(dtype)


def reduction_bound(terms64, chain):
    return chain * U32 * float(terms64.abs().sum())


# ---------------------------------------------------------------------------------------------------------------- Adam
AdamCase = namedtuple("AdamCase", "name n max_blocks mode wd second betas step skip seed")
ADAM_MUTATIONS = ("second_quad_takes_first_gradient", "quad_high_pair_takes_low_pair", "tail_skips_weight_decay", "eps_inside_sqrt", "v_unsquared")
ADAM_DEFAULT_N = (1, 2, 3, 4, 5, 7, 1023, 1024, 1027)
ADAM_CAPPED = ((4 * (256 + 10) + 1, 1), (4 * (512 + 10) + 2, 1), (4 * (1024 + 512 + 100) + 3, 2))
ADAM_MODES = ("host", "host_coef", "device")         # step >= 1 with coef None / a one-element coef; step = 0 with the device sched
ADAM_BETAS = ((0.9, 0.999), (0.9, 0.98))
ADAM_LR, ADAM_EPS = 1e-3, 1e-8


def _adam_cases():
    out = []

    def add(n, mb, mode, wd, second, i, skip=False):
        out.append(AdamCase(f"adam n{n} mb{mb} {mode} wd{wd} {'second' if second else 'first'}{' skip' if skip else ''}", n, mb, mode, wd, second,
                            ADAM_BETAS[i % 2], 1 + 2 * (i % 3) + (10 if second else 0), skip, 7000 + len(out)))

    for i, n in enumerate(ADAM_DEFAULT_N):
        add(n, 0, ADAM_MODES[i % 3], (0.0, 0.01)[i % 2], i % 4 < 2, i)
    for j, (n, mb) in enumerate(ADAM_CAPPED):
        for i, mode in enumerate(ADAM_MODES):
            for wd in (0.0, 0.01):
                add(n, mb, mode, wd, (i + j + (wd > 0)) % 2 == 0, i + j)
    n, mb = ADAM_CAPPED[2]
    add(n, mb, "device", 0.01, True, 1, skip=True)
    return out


ADAM_CASES = _adam_cases()


def f32(x):
    return float(np.float32(x))


def adam_step_size(lr, b1, b2, t):
    """ofa_adam_step's host arithmetic: float(lr sqrt(1 - b2^t) / (1 - b1^t)) on the fp32 lr and betas, in double."""
    lr, b1, b2 = f32(lr), f32(b1), f32(b2)
    return f32(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def adam_plant_positions(n, max_blocks):
    """The four elements of the first k = 1 quad (quad `stride`) and of the last quad before the tail."""
    stride, nq = adam_grid(n, max_blocks) * 256, n >> 2
    return [q for q in (stride, nq - 1) if 0 <= q < nq]


def build_adam(case, dtype, device="cpu"):
    gen, n = _gen(case.seed), case.n
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) + 0.001 * torch.arange(n)            # distinct per element
    for q in adam_plant_positions(n, case.max_blocks):
        g[4 * q:4 * q + 4] = PLANT + torch.arange(4.0)
    if case.second:
        m, v = 0.1 * torch.randn(n, generator=gen), (0.1 * torch.randn(n, generator=gen)) ** 2
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    gmul = 1.0 if case.mode == "host" else 0.37
    b1, b2 = case.betas
    step_size = adam_step_size(ADAM_LR, b1, b2, case.step)
    sched = torch.tensor([gmul, step_size, f32(ADAM_LR), 1.0 if case.skip else 0.0, 0.0])
    coef = None if case.mode == "host" else (sched[:1].clone() if case.mode == "host_coef" else sched)
    d = dict(p=p, m=m, v=v, g=g.to(dtype), coef=coef, gmul=f32(gmul), lr=f32(ADAM_LR), b1=f32(b1), b2=f32(b2), eps=f32(ADAM_EPS), wd=f32(case.wd),
             step_size=step_size, step=0 if case.mode == "device" else case.step)
    return {k: (t.to(device) if torch.is_tensor(t) else t) for k, t in d.items()}


def adam_reference(p, m, v, g, coef, lr, b1, b2, eps, wd, step_size):
    """float64, every scalar the fp32 value the kernel receives -> (ref, bound) over m, v, p.
    g' = g coef[0];  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2;  p' = p - wd lr p - step_size m' / (sqrt(v') + eps)."""
    for b in (b1, b2):
        assert f32(b) == b and float(np.float32(1.0) - np.float32(b)) == 1.0 - b, ("1 - beta is not exact in fp32", b)
    p, m, v, g = p.double(), m.double(), v.double(), g.double() * coef
    m1, m1b = b1 * m + (1 - b1) * g, (b1 * m).abs() + ((1 - b1) * g).abs()
    v1, v1b = b2 * v + (1 - b2) * g * g, (b2 * v).abs() + (1 - b2) * g * g
    upd = step_size * m1 / (v1.sqrt() + eps)
    return dict(m=m1, v=v1, p=p - wd * lr * p - upd), dict(m=m1b, v=v1b, p=p.abs() + wd * lr * p.abs() + upd.abs())


def adam_emulate(b, dtype, max_blocks=0, mutation=None):
    """float32 with adam_kernel's operations in its order -> dict(m, v, p fp32, model of dtype)."""
    assert mutation is None or mutation in ADAM_MUTATIONS, mutation
    n = b["p"].numel()
    nq, stride = n >> 2, adam_grid(n, max_blocks) * 256
    t32 = lambda x: torch.tensor(x, dtype=F32)                              # noqa: E731
    g = b["g"].float().clone()
    if mutation == "second_quad_takes_first_gradient":                       # quad q0 + stride of a trip is fed the gradient of q0
        q = torch.arange(nq)
        src = torch.where((q // stride) % 2 == 1, q - stride, q)
        g[:4 * nq] = g[:4 * nq].view(nq, 4)[src].reshape(-1)
    if mutation == "quad_high_pair_takes_low_pair" and dtype != F32:
        gq = g[:4 * nq].view(nq, 4).clone()
        gq[:, 2:] = gq[:, :2]
        g[:4 * nq] = gq.reshape(-1)
    g = g * t32(b["gmul"])
    b1, b2, lr, eps, wd, ss = (t32(b[k]) for k in ("b1", "b2", "lr", "eps", "wd", "step_size"))
    m = b["m"] * b1 + (t32(1.0) - b1) * g
    v = b["v"] * b2 + (t32(1.0) - b2) * g * (1.0 if mutation == "v_unsquared" else g)
    p = b["p"].clone()
    if float(wd) != 0.0:
        decayed = p - wd * lr * p
        if mutation == "tail_skips_weight_decay":
            decayed[4 * nq:] = p[4 * nq:]
        p = decayed
    den = torch.sqrt(v + eps) if mutation == "eps_inside_sqrt" else torch.sqrt(v) + eps
    p = p - ss * m / den
    return dict(m=m, v=v, p=p, model=p.to(dtype))


def adam_figures(b, got):
    """error / bound of m, v and the master weights; `model`: 0 iff the model copy is round_to_dtype(got's own master) bit for bit."""
    ref, bd = adam_reference(b["p"], b["m"], b["v"], b["g"], b["gmul"], b["lr"], b["b1"], b["b2"], b["eps"], b["wd"], b["step_size"])
    fig = {k: excess(got[k], ref[k], bd[k], 1.0, 2.0 ** -126) for k in ("m", "v", "p")}
    fig["model"] = 0.0 if same_bits(got["model"], got["p"].to(got["model"].dtype)) else float("inf")
    return fig


def adam_limit(name, is_kernel=True):
    return 0.0 if name == "model" else limit("adam", name, F32, is_kernel)
