"""Thin functional wrappers over the C ABI (no autograd here -- see ofasys_amd/ops.py).

Each wrapper allocates outputs with torch (plumbing: device memory + streams), checks layout, and enqueues the HIP
kernel on torch's current stream.  Everything here requires GPU tensors; nothing falls back to torch math.
"""
import contextlib
import ctypes

import torch

from .lib import (BF16, F16, F32, GEMM_ACCUM, GEMM_BIAS_COL, GEMM_BIAS_ROW, GEMM_FORCE_SIMPLE, GEMM_OUT_F32, OfaError,
                  dptr, dtype_code, lib, ptr, stream)

_ws_cache = {}


def workspace(nbytes, device, tag="ws"):
    """A grow-only scratch buffer (fp32 words) per (tag, device, HIP stream): kernels on different streams never share one."""
    key = (tag, device, torch.cuda.current_stream().cuda_stream if device.type == "cuda" else 0)
    buf = _ws_cache.get(key)
    n = (nbytes + 3) // 4
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(n, 1 << 20), dtype=torch.float32, device=device)
        _ws_cache[key] = buf
    return buf


@contextlib.contextmanager
def capture_workspaces(cache):
    """For the duration of a graph capture, workspace() sees only `cache`: the scratch of the owner's earlier captures.  Every
    capture runs on torch's one default capture stream, and a buffer allocated inside a capture lives in that capture's private
    pool: left in the shared cache, a later capture of another owner would address it without owning it and fault once it is
    dropped and the pool released.  On exit `cache` also holds what the capture allocated, the shared cache is back, and the
    yielded dict holds the new buffers alone -- the owner keeps them alive for as long as its graphs."""
    global _ws_cache
    saved, _ws_cache = _ws_cache, dict(cache)
    added = {}
    try:
        yield added
    finally:
        added.update({k: v for k, v in _ws_cache.items() if cache.get(k) is not v})
        cache.update(added)
        _ws_cache = saved


class _FoldJob(ctypes.Structure):
    _fields_ = [("part", ctypes.c_void_p), ("out", ctypes.c_void_p), ("cols", ctypes.c_int64), ("stride", ctypes.c_int64),
                ("nslots", ctypes.c_int32), ("accumulate", ctypes.c_int32), ("alpha", ctypes.c_float),
                ("out_dtype", ctypes.c_int32)]


class _CopyJob(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("bytes", ctypes.c_int64)]


def copy_batched(pairs):
    """dst.copy_(src) for every (dst, src) pair of same-shape, same-dtype, contiguous device tensors -- in ONE launch per 96 pairs
    (ofa_copy_batched).  Pairs that do not qualify are copied by torch."""
    jobs = []
    for dst, src in pairs:
        if (src.dtype == dst.dtype and src.shape == dst.shape and src.device == dst.device and dst.is_cuda
                and src.is_contiguous() and dst.is_contiguous()):
            jobs.append((dptr(src), dptr(dst), src.numel() * src.element_size()))
        else:
            dst.copy_(src, non_blocking=True)
    if jobs:
        arr = (_CopyJob * len(jobs))()
        for it, (s_, d_, n) in zip(arr, jobs):
            it.src, it.dst, it.bytes = s_, d_, n
        lib().call("ofa_copy_batched", ctypes.addressof(arr), len(jobs), stream())


def zero_batched(bufs):
    """Zero fill of every (device address, bytes) in `bufs` in ONE launch per 96 (ofa_zero_batched)."""
    if bufs:
        arr = (_CopyJob * len(bufs))()
        for it, (d_, n) in zip(arr, bufs):
            it.src, it.dst, it.bytes = None, d_, n
        lib().call("ofa_zero_batched", ctypes.addressof(arr), len(bufs), stream())


# First-touch gradient writes.  A launch that ADDS its result to `out` (accumulate=True) asks `grad_mode(out, full)` -- installed by
# ops.py, which keeps the step's touched set -- at the moment it is issued: False = this launch is the first full writer of that
# gradient-arena view in the step and STORES (what is there is not read); True = add.  full=False: the launch writes only part of
# `out`.  Outputs that are no arena gradient (and everything outside a train step) always add.  None: nothing installed, always add.
grad_mode = None


def _accum(out, accumulate, full=True):
    if grad_mode is None:
        return bool(accumulate)
    if accumulate:
        return bool(grad_mode(out, full))
    grad_mode(out, full, store=True)                 # a plain store into an arena gradient is a writer too: the range is marked
    return False


def _accum_all(outs):
    """_accum for a launch with ONE accumulate flag over several gradient outputs: they store only together (an output that alone
    would have stored is cleared first and added to)."""
    if grad_mode is None:
        return True
    if all(grad_mode(o, True, peek=True) is False for o in outs):
        for o in outs:
            grad_mode(o, True)
        return False
    for o in outs:                                   # mixed: each asks as a partial writer (cleared on demand, learned for the next step)
        grad_mode(o, False)
    return True


DEFER_FOLD = 2            # OFA_DEFER_FOLD
FOLD_LANES16 = 4          # OFA_FOLD_LANES16
GEMM_DEFER_REDUCE = 128   # OFA_GEMM_DEFER_REDUCE


class FoldQueue:
    """Deferred `out (+)= alpha * sum_s part[s]` reductions (LayerNorm dgamma/dbeta/dbias, bias column sums, split-K weight
    gradients): producers leave their fp32 partial rows in a private buffer and register a job; `flush()` folds up to 56
    jobs per launch (csrc/fold.hip) instead of one 5-9 us launch each."""

    # partial rows are folded while they still sit in the 256 MiB Infinity Cache: deferring a whole backward pass worth
    # of split-K slabs (3.6 GB on cfg-2) sends them to HBM and back and costs more than the saved launches
    MAX_PENDING_BYTES = 48 << 20        # (one layer's grouped weight-gradient slabs: 12.20 ms/step; 96 MiB 12.25, 200 MiB 12.35, 16 MiB 12.29)

    def __init__(self):
        self.jobs, self.keep, self.bytes, self.outs, self.want_flush = [], [], 0, set(), False
        self.modes = []                              # per job: (accumulate asked for, the other flag bits)

    def add(self, part, part_off, out, cols, stride, nslots, alpha=1.0, accumulate=True, flush_ok=True, lanes16=False):
        """lanes16: sum the slots in the order of ofa_colsum's own final pass (OFA_FOLD_LANES16)."""
        assert part.dtype == torch.float32 and out.is_contiguous()
        if out.data_ptr() in self.outs:
            # a second contribution to the same gradient (a module applied to several slots): jobs of one launch run
            # concurrently, so two read-modify-writes of one output must not share a launch
            self.flush()
        self.outs.add(out.data_ptr())
        self.jobs.append(_FoldJob(dptr(part) + part_off * 4, dptr(out), cols, stride, nslots,
                                  int(bool(accumulate)) | (FOLD_LANES16 if lanes16 else 0), float(alpha), dtype_code(out)))
        self.modes.append((bool(accumulate), FOLD_LANES16 if lanes16 else 0))
        self.keep.append((part, out))
        self.bytes += nslots * stride * 4
        self.want_flush = self.bytes > self.MAX_PENDING_BYTES

    def flush_if_large(self):
        """Called by a producer AFTER it has launched the kernel that writes the partial rows it just registered."""
        if getattr(self, "want_flush", False):
            self.flush()

    def flush(self):
        if not self.jobs:
            return
        for job, (_, out), (want, bits) in zip(self.jobs, self.keep, self.modes):     # store or add: decided HERE, where the launch is issued
            job.accumulate = int(_accum(out, want)) | bits
        arr = (_FoldJob * len(self.jobs))(*self.jobs)
        lib().call("ofa_fold_batched", ctypes.addressof(arr), len(self.jobs), stream())
        self.jobs, self.keep, self.bytes, self.want_flush = [], [], 0, False   # (same stream: buffers may be reused)
        self.modes = []
        self.outs = set()


class ImmediateFold:
    """The FoldQueue's `add` for a caller whose partial rows are already written and that has no queue to defer to (gradients consumed
    from inside backward: data-parallel bucket all-reduces): one fold launch per job, same arithmetic and summation order."""

    def add(self, part, part_off, out, cols, stride, nslots, alpha=1.0, accumulate=True, flush_ok=True, lanes16=False):
        assert part.dtype == torch.float32 and out.is_contiguous()
        job = (_FoldJob * 1)(_FoldJob(dptr(part) + part_off * 4, dptr(out), cols, stride, nslots,
                                      int(_accum(out, accumulate)) | (FOLD_LANES16 if lanes16 else 0), float(alpha), dtype_code(out)))
        lib().call("ofa_fold_batched", ctypes.addressof(job), 1, stream())

    def flush_if_large(self):
        pass


def _u8(mask):
    """bool/uint8 mask as a contiguous uint8 tensor without a copy when possible."""
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)


def _rows_cols(x):
    cols = x.shape[-1]
    return x.numel() // cols, cols


# ------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, gamma, beta, eps=1e-5, fuse_gelu=False):
    x = x.contiguous()
    rows, cols = _rows_cols(x)
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    lib().call("ofa_gelu_layernorm_fwd" if fuse_gelu else "ofa_layernorm_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(y),
               ptr(mean), ptr(rstd), rows, cols, eps, dtype_code(x), stream())
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, fuse_gelu=False, dgamma=None, dbeta=None, dbias=None, want_dbias=False,
                  fold=None, dres=None):
    """dgamma/dbeta given: the parameter gradients are ACCUMULATED into them (gradient arena); else fresh tensors.
    fuse_gelu + (dbias or want_dbias): also the column sums of dx (gradient of the bias of the Linear feeding the GELU)."""
    dy = dy.contiguous()
    x = x.contiguous()
    rows, cols = _rows_cols(x)
    dx = torch.empty_like(x)
    acc = dgamma is not None
    if not acc:
        dgamma = torch.empty(cols, dtype=gamma.dtype, device=x.device)
        dbeta = torch.empty(cols, dtype=gamma.dtype, device=x.device)
        if want_dbias:
            dbias = torch.empty(cols, dtype=gamma.dtype, device=x.device)
    assert dgamma.dtype == x.dtype and dbeta.dtype == x.dtype and (dbias is None or dbias.dtype == x.dtype)
    wsr = lib().cdll.ofa_layernorm_bwd_ws_rows()
    if fold is not None and acc:
        # deferred: keep this call's partial rows [q][nslots][cols] in a private buffer; FoldQueue.flush() reduces them
        ns = lib().cdll.ofa_layernorm_bwd_slots(rows, cols, dtype_code(x), int(fuse_gelu))
        nq = 3 if (fuse_gelu and dbias is not None) else 2
        ws = torch.empty(nq * ns * cols, dtype=torch.float32, device=x.device)
        for q, o in enumerate((dgamma, dbeta, dbias)[:nq]):
            fold.add(ws, q * ns * cols, o, cols, cols, ns)
        acc = DEFER_FOLD
    else:
        ws = workspace(wsr * cols * 4, x.device, "ln")
        if acc:
            acc = _accum_all([o for o in (dgamma, dbeta, dbias if fuse_gelu else None) if o is not None])
    if fuse_gelu:
        lib().call("ofa_gelu_layernorm_bwd", ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dgamma),
                   ptr(dbeta), ptr(dbias), ptr(ws), rows, cols, int(acc), dtype_code(x), stream())
    else:
        if dres is not None:
            dres = dres.contiguous()
            assert dres.shape == x.shape and dres.dtype == x.dtype
        lib().call("ofa_layernorm_bwd", ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(dgamma),
                   ptr(dbeta), ptr(ws), rows, cols, int(acc), dtype_code(x), stream())
    if acc == DEFER_FOLD:
        fold.flush_if_large()
    return dx, dgamma, dbeta, (dbias if fuse_gelu else None)


# ------------------------------------------------------------------ GEMM
def gemm(a, b, trans_a=False, trans_b=False, bias=None, bias_row=False, alpha=1.0, out=None, accumulate=False,
         out_f32=False, force_simple=False, a_kpad_zero=False, fold=None):
    """C = alpha * (op(a) @ op(b) + bias) [+ C].  a, b: 2-D (or 3-D batched) tensors whose last dim is contiguous."""
    assert a.dim() == b.dim() and a.dim() in (2, 3)
    batched = a.dim() == 3
    if a.stride(-1) != 1:
        a = a.contiguous()
    if b.stride(-1) != 1:
        b = b.contiguous()
    batch = a.shape[0] if batched else 1
    ar, ac = a.shape[-2], a.shape[-1]
    br, bc = b.shape[-2], b.shape[-1]
    M, K = (ac, ar) if trans_a else (ar, ac)
    N, Kb = (br, bc) if trans_b else (bc, br)
    if K != Kb:
        raise OfaError(f"gemm: inner dimensions differ ({K} vs {Kb})")
    dt = dtype_code(a)
    if b.dtype != a.dtype:
        raise OfaError("gemm: operand dtypes differ")
    if out is None:
        odt = torch.float32 if (out_f32 or a.dtype == torch.float32) else a.dtype
        out = torch.empty((batch, M, N) if batched else (M, N), dtype=odt, device=a.device)
    flags = 0
    if bias is not None:
        flags |= GEMM_BIAS_ROW if bias_row else GEMM_BIAS_COL
    if accumulate:
        flags |= GEMM_ACCUM
    if force_simple:
        flags |= GEMM_FORCE_SIMPLE
    if dt != F32 and out.dtype == torch.float32:
        flags |= GEMM_OUT_F32
    if a_kpad_zero:
        flags |= 32   # OFA_GEMM_A_KPAD_ZERO
    lda, ldb, ldc = a.stride(-2), b.stride(-2), out.stride(-2)
    sa = a.stride(0) if batched else 0
    sb = b.stride(0) if batched else 0
    sc = out.stride(0) if batched else 0
    ws = None
    if fold is not None and bias is None and not batched and ldc == N and N % 4 == 0 and _prof is None:
        # split-K product whose result nobody reads yet (a weight gradient): leave the fp32 slabs [splits][M][N] in a
        # private buffer and let the FoldQueue reduce them (+ alpha / accumulate) in its batched launch
        nsp = lib().cdll.ofa_gemm_splits(M, N, K, int(trans_a), int(trans_b), 1, flags, dt, 256 << 20)
        if nsp > 1:
            ws = torch.empty(nsp * M * N, dtype=torch.float32, device=a.device)
            fold.add(ws, 0, out, M * N, M * N, nsp, alpha, accumulate)      # (store or add: the fold's decision, at its flush)
            flags |= GEMM_DEFER_REDUCE
            ws_bytes = 256 << 20            # (the planner saw this budget; the slabs themselves fit by construction)
    if ws is None:
        ws = workspace(256 << 20, a.device, "gemm")
        ws_bytes = ws.numel() * 4
        if not _accum(out, accumulate, full=ldc == N and (not batched or sc == M * N)):
            flags &= ~GEMM_ACCUM            # the first full writer of an arena gradient in this step (or a plain store): store
    args = ("ofa_gemm", ptr(a), ptr(b), ptr(out), ptr(bias), M, N, K, int(trans_a), int(trans_b), lda, ldb, ldc, batch,
            sa, sb, sc, 0, 0, 0, 0, float(alpha), flags, dt, ptr(ws), ws_bytes, stream())
    if _prof is not None:
        # roofline timing, IN SITU: two HIP events on the launch stream around THIS launch, inside the running step -- operands
        # as cold / warm as the step leaves them, no re-launch (an eager step is host-bound, so the stream is idle when the kernel
        # starts and the events bracket the kernel alone, + ~1 us of event overhead billed to it)
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        lib().call(*args)
        e1.record()
        _prof.append((2.0 * M * N * K * batch, e0, e1, batch * ((M * K + K * N) * a.element_size() + M * N * out.element_size())))
    else:
        lib().call(*args)
    if flags & GEMM_DEFER_REDUCE:
        fold.flush_if_large()
    return out


def gemm_colstat(a, b, bias=None, max_groups=512):
    """out = a @ b^T (+ bias) like gemm(a, b, False, True), plus the per-column (sum, sum of squares) of the rounded output as partial
    rows [groups, 2, N] fp64 left by the kernel's epilogue (ofa_gemm_colstat), or None when the selected plan cannot produce them."""
    assert a.dim() == 2 and b.dim() == 2 and a.shape[1] == b.shape[1] and a.dtype == b.dtype
    if a.stride(-1) != 1:
        a = a.contiguous()
    if b.stride(-1) != 1:
        b = b.contiguous()
    M, Kd, N = a.shape[0], a.shape[1], b.shape[0]
    out = torch.empty(M, N, dtype=a.dtype, device=a.device)
    if a.dtype == torch.float32 or N % 8:
        return gemm(a, b, False, True, bias=bias, out=out), None
    flags = GEMM_BIAS_COL if bias is not None else 0
    ws = workspace(256 << 20, a.device, "gemm")
    cap = min(max_groups, (M + 31) // 32)
    partial = torch.empty(cap, 2, N, dtype=torch.float64, device=a.device)
    groups = ctypes.c_int(0)
    args = ("ofa_gemm_colstat", ptr(a), ptr(b), ptr(out), ptr(bias), M, N, Kd, 0, 1, a.stride(0), b.stride(0), out.stride(0), 1.0,
            flags, dtype_code(a), ptr(ws), ws.numel() * 4, ptr(partial), cap, ctypes.addressof(groups), stream())
    if _prof is not None:                        # roofline timing in situ (see gemm)
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        lib().call(*args)
        e1.record()
        _prof.append((2.0 * M * N * Kd, e0, e1, (M * Kd + Kd * N + M * N) * a.element_size()))
    else:
        lib().call(*args)
    return out, (partial[:groups.value] if groups.value > 0 else None)


class _GroupItem(ctypes.Structure):     # ofa_gemm_group_item
    _fields_ = [("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("slabs", ctypes.c_void_p), ("lda", ctypes.c_int64),
                ("ldb", ctypes.c_int64), ("m", ctypes.c_int32), ("n", ctypes.c_int32), ("k", ctypes.c_int32),
                ("splits", ctypes.c_int32), ("out", ctypes.c_void_p), ("ldo", ctypes.c_int64), ("out_alpha", ctypes.c_float),
                ("store", ctypes.c_int32)]


GROUP_MAX = 16
GROUP_DIRECT = True      # (tests / A-B tools may clear it: every grouped product then goes through an fp32 slab and the fold)


def gemm_group_ok(dy, x, out):
    """Can out[M,N] (+)= dy[K,M]^T x[K,N] ride in a grouped launch (ofa_gemm_group_tn)?"""
    return (dy.dim() == 2 and x.dim() == 2 and dy.dtype in (torch.bfloat16, torch.float16) and x.dtype == dy.dtype
            and dy.stride(1) == 1 and x.stride(1) == 1 and dy.shape[0] == x.shape[0] and dy.shape[0] >= 1
            and dy.shape[1] % 8 == 0 and x.shape[1] % 8 == 0 and dy.stride(0) % 8 == 0 and x.stride(0) % 8 == 0
            and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and out.is_contiguous())


def gemm_group_tn(products, fold):
    """products: [(dy [K,M], x [K,N], out [M,N], alpha)], each passing gemm_group_ok: out += alpha * dy^T x for all of them in
    ONE launch of 256 x 256 tiles (fp32 K-slice slabs) + the FoldQueue's batched reduce (`fold`: the queue to register the
    slabs with; the caller flushes it)."""
    assert 1 <= len(products) <= GROUP_MAX
    arr = (_GroupItem * len(products))()
    for it, (dy, x, out, alpha) in zip(arr, products):
        it.a, it.b, it.lda, it.ldb = dptr(dy), dptr(x), dy.stride(0), x.stride(0)
        it.m, it.n, it.k = dy.shape[1], x.shape[1], dy.shape[0]
    dt = dtype_code(products[0][0])
    lib().call("ofa_gemm_group_plan", ctypes.addressof(arr), len(products), dt)
    # a product the plan leaves ONE K-slice (a small micro-batch's weight gradients) is accumulated straight onto its 16-bit arena
    # gradient in the kernel's epilogue: no fp32 slab, no fold launch (the fold of a one-slab job only rounds and accumulates).
    # Arithmetic: round(alpha * dY^T X) to 16 bits, add the old 16-bit gradient, round again -- that is the REFERENCE's accumulation
    # over micro-batches (autograd hands AccumulateGrad a 16-bit gradient, `p.grad += g` adds in 16 bits: engine/trainer.py:766-784
    # under model.half() / bfloat16()); the slab + fold path (fp32 sum of the slices and the old gradient, ONE rounding) is tighter than
    # the reference, not the other way round.  tests/test_kernels_gpu.py::test_gemm_group_tn_direct_accumulation_over_micro_batches
    # bounds both against an fp64 sum.
    slabs, direct_outs = [], set()
    for it, (dy, x, out, alpha) in zip(arr, products):
        direct = (GROUP_DIRECT and it.splits == 1 and out.dtype == dy.dtype and out.dim() == 2 and out.stride(1) == 1 and out.stride(0) % 8 == 0
                  and out.data_ptr() % 16 == 0 and out.data_ptr() not in direct_outs)     # (two read-modify-writes of one output
        if direct:                                                                         #  must not share a launch)
            direct_outs.add(out.data_ptr())
            it.out, it.ldo, it.out_alpha = dptr(out), out.stride(0), float(alpha)
            it.store = int(not _accum(out, True, full=out.is_contiguous()))      # (a slab product's fold job decides at its flush)
            slabs.append(None)
        else:
            sl = torch.empty(it.splits * it.m * it.n, dtype=torch.float32, device=dy.device)
            it.slabs = dptr(sl)
            slabs.append(sl)
    if _prof is not None:
        # roofline timing in situ (see gemm): the grouped launch alone; the fold of its K-slice slabs is a FoldQueue launch later on
        # and is accounted for in bench.py from the fold kernel's own share (rocprof), not here
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        lib().call("ofa_gemm_group_tn", ctypes.addressof(arr), len(products), dt, stream())
        e1.record()
        es = products[0][0].element_size()
        _prof.append((sum(2.0 * it.m * it.n * it.k for it in arr), e0, e1,
                      sum((it.m + it.n) * it.k * es + (it.splits * it.m * it.n * 4 if sl is not None else 2 * it.m * it.n * es)
                          for it, sl in zip(arr, slabs))))
    else:
        lib().call("ofa_gemm_group_tn", ctypes.addressof(arr), len(products), dt, stream())
    for it, sl, (dy, x, out, alpha) in zip(arr, slabs, products):   # (registered after the launch: add() may flush the queue)
        if sl is not None:
            fold.add(sl, 0, out, it.m * it.n, it.m * it.n, it.splits, alpha, True)


# ---- optional per-launch timing of the GEMM kernel family (bench.py roofline): HIP events on the launch stream
_prof = None
_PROF_REPS = 1            # (round 1-2 re-launched every call 5x back to back with warm caches; since round 3 the launch itself is timed)


def gemm_profile_begin():
    global _prof
    _prof = []


def gemm_profile_end():
    global _prof
    torch.cuda.synchronize()
    rec, _prof = _prof, None
    return {"launches": len(rec), "flops": sum(r[0] for r in rec), "bytes": sum(r[3] for r in rec),
            "time_ms": sum(r[1].elapsed_time(r[2]) for r in rec) / _PROF_REPS, "reps": _PROF_REPS}


def gemm_heads(a, b, out, M, N, K, trans_a, trans_b, lda, ldb, ldc, B, heads, sa, sa2, sb, sb2, sc, sc2, alpha=1.0,
               accumulate=False):
    """Per-(batch, head) GEMMs straight on [B, T, heads*hd] rows (no permute copies): operand X of product (b, h)
    starts at X + b*sX2 + h*sX."""
    dt = dtype_code(a)
    flags = GEMM_ACCUM if accumulate else 0
    if dt != F32 and out.dtype == torch.float32:
        flags |= GEMM_OUT_F32
    ws = workspace(256 << 20, a.device, "gemm")
    lib().call("ofa_gemm", ptr(a), ptr(b), ptr(out), None, M, N, K, int(trans_a), int(trans_b), lda, ldb, ldc, B * heads,
               sa, sb, sc, heads, sa2, sb2, sc2, float(alpha), flags, dt, ptr(ws), ws.numel() * 4, stream())
    return out


# ------------------------------------------------------------------ softmax family
# (the reference's three pybind extensions, fused_kernels/fused_softmax.py:12-92: forward(inputs, [mask,] scale) and
#  backward(output_grads, softmax_results, scale), fp32 / bf16 / fp16)
def scaled_softmax(x, scale):
    x = x.contiguous()
    b, np_, sq, sk = x.shape
    y = torch.empty_like(x)
    lib().call("ofa_scaled_softmax_fwd", ptr(x), ptr(y), float(scale), b, np_, sq, sk, dtype_code(x), stream())
    return y


def scaled_softmax_bwd(dy, y, scale, inplace=False):
    dy = dy.contiguous()
    y = y.contiguous()
    rows = y.numel() // y.shape[-1]
    dx = dy if inplace else torch.empty_like(dy)
    lib().call("ofa_scaled_softmax_bwd", ptr(dy), ptr(y), ptr(dx), float(scale), 1, 1, rows, y.shape[-1], dtype_code(y),
               stream())
    return dx


def scaled_masked_softmax(x, mask, scale):
    x = x.contiguous()
    mask = mask.to(torch.uint8).contiguous()
    b, np_, sq, sk = x.shape
    y = torch.empty_like(x)
    lib().call("ofa_scaled_masked_softmax_fwd", ptr(x), ptr(mask), ptr(y), float(scale), b, np_, sq, sk, mask.shape[0],
               dtype_code(x), stream())
    return y


def scaled_masked_softmax_bwd(dy, y, scale, inplace=True):
    """In place on dy by default, as the reference's extension (scaled_masked_softmax_cuda.cu:98-117)."""
    assert dy.is_contiguous() and y.is_contiguous() and dy.shape == y.shape and y.dim() == 4
    b, np_, sq, sk = y.shape
    dx = dy if inplace else torch.empty_like(dy)
    lib().call("ofa_scaled_masked_softmax_bwd", ptr(dy), ptr(y), ptr(dx), float(scale), b, np_, sq, sk, dtype_code(y),
               stream())
    return dx


def scaled_upper_triang_masked_softmax(x, scale):
    x = x.contiguous()
    ab, sq, sk = x.shape
    assert sq == sk
    y = torch.empty_like(x)
    lib().call("ofa_scaled_upper_triang_masked_softmax_fwd", ptr(x), ptr(y), float(scale), ab, sq, dtype_code(x), stream())
    return y


def scaled_upper_triang_masked_softmax_bwd(dy, y, scale, inplace=True):
    """In place on dy by default (scaled_upper_triang_masked_softmax_cuda.cu:68-95); dx is zero above the diagonal."""
    assert dy.is_contiguous() and y.is_contiguous() and dy.shape == y.shape and y.dim() == 3 and y.shape[1] == y.shape[2]
    dx = dy if inplace else torch.empty_like(dy)
    lib().call("ofa_scaled_upper_triang_masked_softmax_bwd", ptr(dy), ptr(y), ptr(dx), float(scale), y.shape[0], y.shape[1],
               dtype_code(y), stream())
    return dx


def get_batch_per_block(sq, sk, b, np_):
    return lib().cdll.ofa_get_batch_per_block(sq, sk, b, np_)


def attn_softmax(x, bias, kpm, scale, heads, causal):
    x = x.contiguous()
    BA, T, S = x.shape
    if bias is not None:
        bias = bias.contiguous()
    if kpm is not None:
        kpm = _u8(kpm)
    p = torch.empty_like(x)
    lib().call("ofa_attn_softmax_fwd", ptr(x), ptr(bias), ptr(kpm), ptr(p), float(scale), BA, heads, T, S, int(causal),
               dtype_code(x), stream())
    return p


# ------------------------------------------------------------------ fused attention (bf16)
def pad32(n):
    return (n + 31) // 32 * 32


def transpose_heads(x, T_pad):
    """x: [B, T, C] (last dim contiguous) -> [B, C, T_pad], zero for t >= T."""
    B, T, C = x.shape
    if x.stride(-1) != 1 or x.stride(0) != T * x.stride(1):
        x = x.contiguous()
    xt = torch.empty(B, C, T_pad, dtype=x.dtype, device=x.device)
    lib().call("ofa_transpose_heads", ptr(x), ptr(xt), B, T, C, T_pad, x.stride(1), dtype_code(x), stream())
    return xt


def _rows3(x):
    """[B, T, D] view with contiguous last dim and dense batch stride; returns (tensor, ld)."""
    if x.stride(-1) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
        x = x.contiguous()
    return x, x.stride(1)


def _same_ld(k, v):
    k, ldk = _rows3(k)
    v, ldv = _rows3(v)
    if ldv != ldk:
        k, v = k.contiguous(), v.contiguous()
        ldk = k.stride(1)
    return k, v, ldk


def _c_dtype(c_attn):
    """dtype code of the per-head scale (fp32 or bf16 [heads], contiguous); fp32 when absent."""
    if c_attn is None:
        return dtype_code(torch.empty(0, dtype=torch.float32))
    assert c_attn.is_contiguous()
    return dtype_code(c_attn)


def c_attn_grad(delta, c_attn, B, heads, T, out=None, accumulate=False):
    """d c_attn[h] = sum_{b,t<T} delta[b*heads+h, t] / c_attn[h]  (delta: fp32 [B*heads, ld] from attn_bwd)."""
    if out is None:
        out = torch.empty_like(c_attn)
        accumulate = False
    lib().call("ofa_c_attn_grad", ptr(delta), ptr(c_attn), ptr(out), B, heads, T, delta.stride(0), int(_accum(out, accumulate)),
               dtype_code(c_attn), stream())
    return out


def _shared_bias(bias, heads, q):
    """A batch-shared position bias: [heads, Tb, Sb] (the reference's [B*A, T, S] tensor is B copies of it), contiguous, q's dtype."""
    assert bias.dim() == 3 and bias.shape[0] == heads, (tuple(bias.shape), heads)
    if bias.dtype != q.dtype:
        bias = bias.to(q.dtype)
    return bias.contiguous()


class _BiasSlots(ctypes.Structure):
    _fields_ = [("values", ctypes.c_void_p * 8), ("values2", ctypes.c_void_p * 8), ("start", ctypes.c_int32 * 8), ("n", ctypes.c_int32 * 8),
                ("inner", ctypes.c_int32 * 8), ("count", ctypes.c_int32)]


def bias_build(abs_bias, starts=(), values=(), heads=None, want_out=True):
    """The batch-shared position bias of one layer (ofa_bias_build): out = abs_bias [A, Tb, Sb] (None: zeros) with values_k
    [n_k, n_k, A] added on the diagonal block at starts[k] -> (out [A, Tb, Sb] or None, (row image, column image)): the two
    tile-swizzled images the shared-bias attention kernels read."""
    live = [(s, v) for s, v in zip(starts, values) if v is not None]
    ref = abs_bias if abs_bias is not None else (live[0][1][0] if isinstance(live[0][1], tuple) else live[0][1])
    slots = _BiasSlots()
    assert len(live) <= 8, "at most 8 slots per bias"
    keep, ends = [], []
    for i, (s, v) in enumerate(live):
        if isinstance(v, tuple):             # an OUTER slot (frames [F,F,A], patches [P,P,A]): value(i, j) = frames[i/P][j/P] + patches[i%P][j%P]
            vf, vi = (t.to(ref.dtype).contiguous() for t in v)
            keep += [vf, vi]
            n = vf.shape[0] * vi.shape[0]
            slots.values[i], slots.values2[i], slots.inner[i] = dptr(vf), dptr(vi), vi.shape[0]
        else:
            v = v.to(ref.dtype).contiguous()
            keep.append(v)
            n = v.shape[0]
            slots.values[i], slots.values2[i], slots.inner[i] = dptr(v), None, 0
        slots.start[i], slots.n[i] = int(s), n
        ends.append(int(s) + n)
    slots.count = len(live)
    if abs_bias is not None:
        abs_bias = abs_bias.contiguous()
        A, Tb, Sb = abs_bias.shape
    else:
        A = heads
        Tb = Sb = max(ends)
    n = lib().cdll.ofa_bias_swz_elems(A, Tb, Sb)
    swz = torch.empty(2, n, dtype=ref.dtype, device=ref.device)
    out = torch.empty(A, Tb, Sb, dtype=ref.dtype, device=ref.device) if want_out else None
    lib().call("ofa_bias_build", ptr(abs_bias), ctypes.addressof(slots), ptr(out), ptr(swz[0]), ptr(swz[1]), A, Tb, Sb,
               dtype_code(ref), stream())
    return out, (swz[0], swz[1])


def _shared_swz(bias, bias_shared):
    """bias_shared: True (the images are built here, one extra launch) or the (row image, column image) pair of bias_build."""
    if isinstance(bias_shared, tuple):
        return bias_shared
    return bias_build(bias, want_out=False)[1]


class _AttnCall(ctypes.Structure):     # ofa_attn_call
    _fields_ = ([(n, ctypes.c_void_p) for n in ("q k v dout out lse delta dq dk dv bias bias_swz_row bias_swz_col dbias ws kpm c_attn seg "
                                                "cs_q cs_k cs_v cs_c").split()]
                + [(n, ctypes.c_int64) for n in "ldq ldk ldo ws_bytes cs_ldq cs_ldk".split()]
                + [(n, ctypes.c_int32) for n in "B heads T S Tpad Tb Sb causal rows_q rows_k dtype c_attn_dtype dbias_dtype".split()]
                + [("scale", ctypes.c_float)])


def _attn_call(q, k, v, heads, scale, bias, kpm, c_attn, causal, seg, bias_shared, dense_grads=False):
    """The part of an ofa_attn_call the forward and the backward share -> (call, q, k, v, bias, swz): the operands as the kernels read
    them, the shared bias as [heads, Tb, Sb] with its (row image, column image) pair.  call.keep holds every tensor the call points at.
    dense_grads: the backward allocates dq / dk / dv itself -- dq is written with ld = ldq, dk / dv with ld = ldk, so dense strides
    give it dense outputs."""
    q, ldq = _rows3(q)
    k, v, ldk = _same_ld(k, v)
    B, T, D = q.shape
    S = k.shape[1]
    if dense_grads and ldq != D:
        q, ldq = q.contiguous(), D
    if dense_grads and ldk != D:
        k, v, ldk = k.contiguous(), v.contiguous(), D
    c, swz = _AttnCall(), None
    c.q, c.k, c.v, c.c_attn, c.c_attn_dtype = ptr(q), ptr(k), ptr(v), ptr(c_attn), _c_dtype(c_attn)
    c.heads, c.Tpad, c.ldq, c.ldk, c.scale, c.causal, c.dtype = heads, pad32(T), ldq, ldk, float(scale), int(causal), dtype_code(q)
    c.B, c.T, c.S = B, T, S
    if bias_shared:
        bias = _shared_bias(bias, heads, q)
        c.Tb, c.Sb = Tb, Sb = bias.shape[1], bias.shape[2]
        swz = _shared_swz(bias, bias_shared)
        c.bias_swz_row = ptr(swz[0])                        # (the forward reads the row image alone)
    elif bias is not None:
        bias = bias.contiguous()
        c.bias = ptr(bias)
    if seg is not None:
        assert B == 1 and kpm is None and seg.rows_q == T and seg.rows_k == S, (B, T, S, seg.rows_q, seg.rows_k)
        assert (bias is None) if not bias_shared else (Tb >= seg.max_q - 31 and Sb >= seg.max_k - 31)
        c.B, c.T, c.S = seg.batch, seg.max_q, seg.max_k
        if bias_shared:
            c.T, c.S = min(seg.max_q, Tb), min(seg.max_k, Sb)
        c.seg, c.rows_q, c.rows_k = ptr(seg.table), T, S
    elif kpm is not None:
        kpm = _u8(kpm)
        c.kpm = ptr(kpm)
    c.keep = [q, k, v, c_attn, bias, swz, kpm, seg]
    return c, q, k, v, bias, swz


def attn_fwd(q, k, v, heads, scale, bias=None, kpm=None, c_attn=None, causal=False, seg=None, bias_shared=False):
    """q [B,T,D], k, v [B,S,D] (row views of a packed buffer are fine) -> out [B,T,D], lse [B*heads, Tpad].
    seg (packing.Segments): ragged mode -- q [1,rows_q,D], k, v [1,rows_k,D] hold the samples back to back, out rows outside
    every segment are zero (the kernel writes them), lse is [heads, pad32(rows_q)] by packed row.
    bias_shared: bias is [heads, Tb, Sb], the same for every sample, indexed by the position inside the sample."""
    c, q = _attn_call(q, k, v, heads, scale, bias, kpm, c_attn, causal, seg, bias_shared)[:2]
    B, T, D = q.shape
    out = torch.empty(B, T, D, dtype=q.dtype, device=q.device)
    lse = torch.empty(B * heads, c.Tpad, dtype=torch.float32, device=q.device)
    c.out, c.lse, c.ldo = ptr(out), ptr(lse), D
    lib().call("ofa_attn_fwd", ctypes.addressof(c), stream())
    return out, lse


def attn_cs_slots(B, T, seg=None, k_side=False):
    """Partial rows of the column sums the attention backward kernels leave per call (ofa_attn_call.cs_*): one per (sample, 128-row tile)."""
    if seg is not None:
        B, T = seg.batch, (seg.max_k if k_side else seg.max_q)
    return lib().cdll.ofa_attn_cs_slots(int(B), int(T))


def _cs_args(c, cs, heads):
    """cs = dict(q=, k=, v=, c=): fp32 2-D views [slots, heads * 64] (row stride free, k and v the same; c: [slots, heads] contiguous)."""
    q, k, v, cc = cs.get("q"), cs.get("k"), cs.get("v"), cs.get("c")
    for t in (q, k, v):
        assert t is None or (t.dtype == torch.float32 and t.stride(1) == 1 and t.shape[1] == heads * 64)
    assert cc is None or (cc.dtype == torch.float32 and cc.is_contiguous() and cc.shape[1] == heads)
    assert k is None or v is None or k.stride(0) == v.stride(0)
    kv = k if k is not None else v
    c.cs_q, c.cs_k, c.cs_v, c.cs_c = ptr(q), ptr(k), ptr(v), ptr(cc)
    c.cs_ldq, c.cs_ldk = q.stride(0) if q is not None else 0, kv.stride(0) if kv is not None else 0


def attn_bwd(q, k, v, out, dout, lse, heads, scale, bias=None, kpm=None, c_attn=None, causal=False, need_dbias=False,
             outs=None, seg=None, bias_shared=False, dbias_dtype=torch.float32, cs=None):
    """outs=(dq, dk, dv): caller-provided gradient views with the SAME row strides as q / k (e.g. column slices of one
    packed [B,T,3D] buffer next to a packed qkv input) -- the kernels write them in place.
    cs: optional dict of fp32 partial-row buffers (see _cs_args / attn_cs_slots) that receive the column sums of dq / dk / dv and
    the per-head sums of delta / c_attn -- the projections' bias gradients and the c_attn gradient, finished by the FoldQueue."""
    c, q, k, v, bias, swz = _attn_call(q, k, v, heads, scale, bias, kpm, c_attn, causal, seg, bias_shared, dense_grads=outs is None)
    dout, ldo = _rows3(dout)
    out, ldo2 = _rows3(out)
    if ldo != ldo2:
        dout, out = dout.contiguous(), out.contiguous()
        ldo = dout.stride(1)
    B, T, D = q.shape
    S = k.shape[1]
    delta = torch.empty(B * heads, c.Tpad, dtype=torch.float32, device=q.device)   # rowsum(dO*O): written by the dQ kernel
    dbias = ws = None
    if need_dbias and not bias_shared:
        assert seg is None
        dbias = torch.empty(B * heads, T, S, dtype=q.dtype, device=q.device)
    if outs is not None:
        dq, dk, dv = outs
        assert dq.stride(1) == c.ldq and dk.stride(1) == c.ldk and dv.stride(1) == c.ldk
    else:
        dq = torch.empty(B, T, D, dtype=q.dtype, device=q.device)     # (ragged mode: the kernels zero the filler rows)
        dk = torch.empty(B, S, D, dtype=q.dtype, device=q.device)
        dv = torch.empty(B, S, D, dtype=q.dtype, device=q.device)
    if cs:
        _cs_args(c, cs, heads)
    if bias_shared:
        c.bias, c.bias_swz_col = ptr(bias), ptr(swz[1])
        if need_dbias:
            # fp32 (or 16-bit: cast by the chunk fold) [heads, Tb, Sb] = the sum over the batch of dS, from the batch-walking third kernel
            dbias = torch.empty(heads, c.Tb, c.Sb, dtype=dbias_dtype, device=q.device)
            c.dbias_dtype = dtype_code(dbias)
            nchunk = lib().cdll.ofa_attn_sbias_chunks(c.B, heads, c.Tb, c.Sb)
            if nchunk > 1 or dbias_dtype not in (torch.float32, q.dtype):
                ws = torch.empty(nchunk, heads, c.Tb, c.Sb, dtype=torch.float32, device=q.device)
                c.ws, c.ws_bytes = ptr(ws), ws.numel() * 4
    c.dout, c.out, c.lse, c.delta, c.ldo = ptr(dout), ptr(out), ptr(lse), ptr(delta), ldo
    c.dq, c.dk, c.dv, c.dbias = ptr(dq), ptr(dk), ptr(dv), ptr(dbias)
    lib().call("ofa_attn_bwd", ctypes.addressof(c), stream())
    return dq, dk, dv, dbias, delta


def attn_decode(q, k_cache, v_cache, S, heads, scale, bias=None, kpm=None, c_attn=None, need_probs=False):
    """One query row per batch entry against a KV cache (csrc/attention_decode.hip).
    q: [B, D]; k_cache, v_cache: [B, capacity, D] (same strides, last dim contiguous), the first S rows valid;
    bias: [B*heads, S] or None; kpm: bool/uint8 [B, >= S] or None.  Returns out [B, D] and probs [B*heads, S] (or None)."""
    B, D = q.shape
    q = q.contiguous()
    assert k_cache.dim() == 3 and k_cache.shape == v_cache.shape and k_cache.stride() == v_cache.stride()
    assert k_cache.stride(2) == 1 and k_cache.shape[0] == B and k_cache.shape[1] >= S and k_cache.dtype == q.dtype
    out = torch.empty(B, D, dtype=q.dtype, device=q.device)
    probs = torch.empty(B * heads, S, dtype=q.dtype, device=q.device) if need_probs else None
    if bias is not None:
        bias = bias.reshape(B * heads, S).to(q.dtype).contiguous()
    kpm_ld = 0
    if kpm is not None:
        kpm = _u8(kpm)
        kpm_ld = kpm.stride(0)
    lib().call("ofa_attn_decode", ptr(q), ptr(k_cache), ptr(v_cache), ptr(bias), ptr(kpm), ptr(c_attn), _c_dtype(c_attn),
               ptr(out), ptr(probs), B, heads, D // heads, S, k_cache.stride(1), k_cache.stride(0), kpm_ld, float(scale),
               dtype_code(q), stream())
    return out, probs


# ------------------------------------------------------------------ elementwise / embedding
def gelu_fwd(x):
    x = x.contiguous()
    y = torch.empty_like(x)
    lib().call("ofa_gelu_fwd", ptr(x), ptr(y), x.numel(), dtype_code(x), stream())
    return y


def gelu_bwd(dy, x):
    dy, x = dy.contiguous(), x.contiguous()
    dx = torch.empty_like(x)
    lib().call("ofa_gelu_bwd", ptr(dy), ptr(x), ptr(dx), x.numel(), dtype_code(x), stream())
    return dx


def quick_gelu_fwd(h):
    """a = h * sigmoid(1.702 h) on [rows, cols] (module/vit.py QuickGELU)."""
    h = h.contiguous()
    rows, cols = _rows_cols(h)
    a = torch.empty_like(h)
    lib().call("ofa_quick_gelu_fwd", ptr(h), ptr(a), rows, cols, dtype_code(h), stream())
    return a


def quick_gelu_bwd_slots(rows, cols, dtype_code_):
    return lib().cdll.ofa_quick_gelu_bwd_slots(int(rows), int(cols), int(dtype_code_))


def quick_gelu_bwd(dy, h, dbias=None, fold=None, want_partials=False):
    """dh of QuickGELU.  dbias (with fold): the column sums of dh -- the bias gradient of the Linear in front -- are ADDED to it: the
    kernel leaves fp32 partial rows and `fold` (a FoldQueue / ImmediateFold) finishes them.  want_partials: -> (dh, partial rows
    [slots, cols]) with nothing folded."""
    dy, h = dy.contiguous(), h.contiguous()
    rows, cols = _rows_cols(h)
    dh = torch.empty_like(h)
    ws = None
    if (dbias is not None or want_partials) and rows > 0:
        ns = quick_gelu_bwd_slots(rows, cols, dtype_code(h))
        ws = torch.empty(ns, cols, dtype=torch.float32, device=h.device)
    lib().call("ofa_quick_gelu_bwd", ptr(dy), ptr(h), ptr(dh), ptr(ws), rows, cols, dtype_code(h), stream())
    if dbias is not None and ws is not None:
        # registered AFTER the launch that writes the partial rows: an ImmediateFold folds at once, a FoldQueue at its flush
        fold.add(ws, 0, dbias, cols, cols, ns)
        fold.flush_if_large()
    return (dh, ws) if want_partials else dh


def dropout_add(x, residual, p, seed, offset, offset_base=None):
    """offset_base: optional device int64[1] added to `offset` on the device (graph-safe Philox stream position)."""
    x = x.contiguous()
    if residual is not None:
        residual = residual.contiguous()
    y = torch.empty_like(x)
    lib().call("ofa_dropout_add_fwd", ptr(x), ptr(residual), ptr(y), x.numel(), float(p), seed, offset, ptr(offset_base),
               dtype_code(x), stream())
    return y


def dropout_bwd(dy, p, seed, offset, offset_base=None):
    dy = dy.contiguous()
    dx = torch.empty_like(dy)
    lib().call("ofa_dropout_bwd", ptr(dy), ptr(dx), dy.numel(), float(p), seed, offset, ptr(offset_base), dtype_code(dy),
               stream())
    return dx


def add_rowvec_mask(a, b=None, vec=None, rowmask=None):
    """b: same rows as a, or the rows of ONE sample (a's row count a multiple of b's: positions shared by the batch)."""
    a = a.contiguous()
    rows, cols = _rows_cols(a)
    period = 0
    if b is not None:
        b = b.contiguous()
        brows = b.numel() // cols
        if brows != rows:
            assert brows > 0 and rows % brows == 0, (rows, brows)
            period = brows
    if rowmask is not None:
        rowmask = _u8(rowmask)
    y = torch.empty_like(a)
    lib().call("ofa_add_rowvec_mask", ptr(a), ptr(b), ptr(vec), ptr(rowmask), ptr(y), rows, cols, period, dtype_code(a), stream())
    return y


def batch_sum(x, batch, out=None, accumulate=False):
    """x [batch * n] (contiguous) -> out [n] = sum over the batch (fp32 accumulation)."""
    x = x.contiguous()
    n = x.numel() // batch
    if out is None:
        out = torch.empty(n, dtype=x.dtype, device=x.device)
        accumulate = False
    lib().call("ofa_batch_sum", ptr(x), ptr(out), int(batch), n, int(_accum(out, accumulate)), dtype_code(x), stream())
    return out


def embedding_fwd(weight, ids, pad_mask_of=None):
    """pad_mask_of: a token id -- also returns the bool mask ids == pad_mask_of, written by the same kernel."""
    ids = ids.contiguous()
    V, D = weight.shape
    out = torch.empty(*ids.shape, D, dtype=weight.dtype, device=weight.device)
    mask = None
    if pad_mask_of is not None and D % (4 if weight.dtype == torch.float32 else 8) == 0:
        mask = torch.empty(ids.shape, dtype=torch.bool, device=weight.device)
    lib().call("ofa_embedding_fwd", ptr(weight), ptr(ids), ptr(out), ids.numel(), D, V, ptr(mask), int(pad_mask_of) if mask is not None else 0,
               dtype_code(weight), stream())
    if pad_mask_of is None:
        return out
    return out, (mask if mask is not None else ids.eq(pad_mask_of))


def gather_rows(src2d, index):
    """out[r] = index[r] >= 0 ? src2d[index[r]] : 0  (index: int64 [n] on the device)."""
    assert src2d.dim() == 2 and src2d.is_contiguous() and index.dtype == torch.int64 and index.is_contiguous()
    out = torch.empty(index.numel(), src2d.shape[1], dtype=src2d.dtype, device=src2d.device)
    lib().call("ofa_gather_rows", ptr(src2d), ptr(index), ptr(out), index.numel(), src2d.shape[1], src2d.shape[0],
               dtype_code(src2d), stream())
    return out


def gather_rows_parts(parts, index):
    """Packed rows of the virtual concatenation torch.cat(parts, dim=1) (parts: contiguous [B, n_k, D], <= 8 of them): index[r] = b * T + t."""
    assert 1 <= len(parts) <= 8 and index.dtype == torch.int64 and index.is_contiguous()
    B, D = parts[0].shape[0], parts[0].shape[2]
    assert all(t.dim() == 3 and t.is_contiguous() and t.shape[0] == B and t.shape[2] == D and t.dtype == parts[0].dtype for t in parts)
    out = torch.empty(index.numel(), D, dtype=parts[0].dtype, device=parts[0].device)
    srcs = (ctypes.c_void_p * len(parts))(*[dptr(t) for t in parts])
    lens = (ctypes.c_int * len(parts))(*[int(t.shape[1]) for t in parts])
    lib().call("ofa_gather_rows_parts", ctypes.addressof(srcs), ctypes.addressof(lens), len(parts), ptr(index), ptr(out), index.numel(), D, B,
               dtype_code(parts[0]), stream())
    return out


def scatter_rows_part(dpacked, inverse, B, nk, Ttot, start):
    """[B, nk, D] gradient of one part: row (b, j) = dpacked[inverse[b * Ttot + start + j]] or 0."""
    assert dpacked.dim() == 2 and dpacked.is_contiguous() and inverse.dtype == torch.int64 and inverse.is_contiguous()
    D = dpacked.shape[1]
    out = torch.empty(B, nk, D, dtype=dpacked.dtype, device=dpacked.device)
    lib().call("ofa_scatter_rows_part", ptr(dpacked), ptr(inverse), ptr(out), B, nk, Ttot, start, D, dpacked.shape[0], dtype_code(dpacked), stream())
    return out


# items of the debug library's OFA_STEP_TAIL_OLD mask (include/ofasys_amd.h: OFA_TAIL_*)
TAIL_FIRST_TOUCH, TAIL_NORM_SCHEDULE, TAIL_CRITERION_STATS = 0, 1, 2


def tail_old(item):
    """Debug library with OFA_STEP_TAIL_OLD set: the gradient plumbing around the optimizer as it ran before (A/B runs); else False."""
    return bool(lib().cdll.ofa_step_tail_old(int(item)))


# items of the debug library's OFA_STEP_EDGES_OLD mask (include/ofasys_amd.h: OFA_EDGE_*)
EDGE_POS_RANGE, EDGE_TOKEN_BWD, EDGE_COLSUM_FOLD, EDGE_IM2COL = 0, 1, 2, 3


def edge_old(item):
    """Debug library with OFA_STEP_EDGES_OLD set: take the path this caller took before its one-launch form (A/B runs); else False."""
    return bool(lib().cdll.ofa_step_edges_old(int(item)))


def embedding_bwd(dout, ids, V, padding_idx=-1, dweight=None, id_major=None):
    """dweight[v] += sum of the rows of dout whose id is v.  id_major: True / False picks the one-launch id-major kernel / the table-row-
    major ones (same bits either way); None: id-major for wide-vocabulary tables (one slice: few hits per row) whose id list fits it."""
    dout = dout.contiguous()
    ids = ids.contiguous()
    D = dout.shape[-1]
    if dweight is None:
        dweight = torch.zeros(V, D, dtype=dout.dtype, device=dout.device)
    else:
        _accum(dweight, True, full=False)            # touches the rows of the ids only: a partial writer always adds
    S = lib().cdll.ofa_embedding_bwd_slices(V, D)
    pad = -1 if padding_idx is None else padding_idx
    if id_major is None:
        id_major = S == 1 and not edge_old(EDGE_TOKEN_BWD)
    if (id_major and lib().cdll.ofa_embedding_bwd_ids_ok(ids.numel(), D, V, dtype_code(dout))
            and (dout.data_ptr() | dweight.data_ptr()) % 16 == 0):
        lib().call("ofa_embedding_bwd_ids", ptr(dout), ptr(ids), ptr(dweight), ids.numel(), D, V, pad, S, dtype_code(dout), stream())
        return dweight
    present = workspace(V, dout.device, "embed_present") if V > 4096 else None
    slices = workspace(S * V * D * 4, dout.device, "embed_slices") if S > 1 else None
    lib().call("ofa_embedding_bwd", ptr(dout), ptr(ids), ptr(dweight), ids.numel(), D, V,
               pad, ptr(present), ptr(slices), dtype_code(dout), stream())
    return dweight


def embedding_range_ok(x):
    """Can ofa_embedding_range_bwd take gradient rows like x's (whole 16-byte vectors)?"""
    return x.shape[-1] % (4 if x.dtype == torch.float32 else 8) == 0 and not edge_old(EDGE_POS_RANGE)


def embedding_range_bwd(dout, dweight, r0, T):
    """dweight[r0 + t] += round(sum_b dout[b, t]): the gradient of the table rows r0 .. r0 + T - 1 a lookup by arange handed to every
    sample, from dout [batch, T, D] (or [T, D]) -- batch sum and scatter-add of the generic route in one pass, the same bits."""
    dout = dout.contiguous()
    V, D = dweight.shape
    batch = dout.numel() // (T * D)
    assert dweight.is_contiguous() and dweight.dtype == dout.dtype and batch * T * D == dout.numel()
    _accum(dweight, True, full=False)                # rows r0 .. r0 + T - 1 only: a partial writer always adds
    lib().call("ofa_embedding_range_bwd", ptr(dout), ptr(dweight), batch, T, D, V, int(r0), dtype_code(dout), stream())
    return dweight


def segment_rowsum(dout2d, plan, dweight, accumulate):
    """dweight[plan.rows[s]] (+)= sum of the rows of dout2d in segment s (ofa_segment_rowsum); plan: ops.SegmentPlan."""
    assert dout2d.dim() == 2 and dout2d.is_contiguous() and dweight.is_contiguous() and dout2d.dtype == dweight.dtype
    if accumulate:
        _accum(dweight, True, full=False)            # the rows of the plan's ids only: a partial writer always adds
    lib().call("ofa_segment_rowsum", ptr(dout2d), ptr(plan.order), ptr(plan.seg_off), ptr(plan.seg_row), ptr(dweight), plan.nseg,
               dout2d.shape[1], int(accumulate), dtype_code(dout2d), stream())
    return dweight


def im2col_patch(img, p, Kpad, lead=0):
    """[B, C, H, W] -> [B * (lead + N), Kpad]: every sample's N patch rows behind `lead` zero rows."""
    img = img.contiguous()
    B, C, H, W = img.shape
    col = torch.empty(B * (lead + (H // p) * (W // p)), Kpad, dtype=img.dtype, device=img.device)
    lib().call("ofa_im2col_patch", ptr(img), ptr(col), B, C, H, W, p, Kpad, int(lead), dtype_code(img), stream())
    return col


# ------------------------------------------------------------------ criterion / optimizer
def step_stats_add(stats, loss, target, pad):
    """stats (fp64 [3]: sample_size, loss_sum, ntokens) += (non-pad targets, loss, non-pad targets): one launch."""
    assert stats.dtype == torch.float64 and stats.numel() >= 3 and loss.dtype == torch.float32 and loss.numel() == 1
    t = target.reshape(-1)
    assert t.dtype == torch.int64 and t.is_contiguous()
    lib().call("ofa_step_stats_add", ptr(stats), ptr(loss), ptr(t), t.numel(), int(pad), stream())


def cross_entropy_fwd(logits2d, target, V, ignore_index):
    """logits2d: [rows, ld] storage (ld >= V, multiple of the vector width); returns lse [rows], row_loss [rows]."""
    rows, ld = logits2d.shape[0], logits2d.stride(0)
    lse = torch.empty(rows, dtype=torch.float32, device=logits2d.device)
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits2d.device)
    lib().call("ofa_cross_entropy_fwd", ptr(logits2d), ptr(target), ptr(lse), ptr(row_loss), rows, V, ld, ignore_index,
               dtype_code(logits2d), stream())
    return lse, row_loss


def cross_entropy_fwd_grad_ok(logits2d, V):
    return logits2d.is_cuda and bool(lib().cdll.ofa_cross_entropy_fwd_grad_ok(int(V), int(logits2d.stride(0)), dtype_code(logits2d)))


def cross_entropy_fwd_grad(logits2d, target, grad_scale, V, ignore_index, stats=None, ticket=None):
    """lse, row_loss AND dlogits = (softmax - onehot) * grad_scale[0] in one pass over the logits (ofa_cross_entropy_fwd_grad):
    grad_scale is the fp32 device scalar the backward pass will be seeded with (None: 1).
    stats (fp64[3]) + ticket (one int32 device word, 0 before the first call): the kernel's last block also sums the row losses and adds
    [non-ignored targets, loss, non-ignored targets] to stats (ofa_cross_entropy_fwd_grad_stats); returns (lse, row_loss, dlogits, loss)."""
    rows, ld = logits2d.shape[0], logits2d.stride(0)
    lse = torch.empty(rows, dtype=torch.float32, device=logits2d.device)
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits2d.device)
    dlogits = torch.empty(rows, ld, dtype=logits2d.dtype, device=logits2d.device)
    if stats is not None:
        assert stats.dtype == torch.float64 and stats.numel() >= 3 and ticket.dtype == torch.int32 and rows >= 1
        assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == rows
        loss = torch.empty((), dtype=torch.float32, device=logits2d.device)
        lib().call("ofa_cross_entropy_fwd_grad_stats", ptr(logits2d), ptr(target), ptr(grad_scale), ptr(lse), ptr(row_loss), ptr(dlogits),
                   rows, V, ld, ignore_index, dtype_code(logits2d), ptr(loss), ptr(stats), ptr(ticket), stream())
        return lse, row_loss, dlogits, loss
    lib().call("ofa_cross_entropy_fwd_grad", ptr(logits2d), ptr(target), ptr(grad_scale), ptr(lse), ptr(row_loss), ptr(dlogits), rows, V,
               ld, ignore_index, dtype_code(logits2d), stream())
    return lse, row_loss, dlogits


def cross_entropy_bwd(logits2d, target, lse, grad_scale, V, ignore_index, dlogits=None):
    rows, ld = logits2d.shape[0], logits2d.stride(0)
    if dlogits is None:
        dlogits = torch.empty(rows, ld, dtype=logits2d.dtype, device=logits2d.device)
    lib().call("ofa_cross_entropy_bwd", ptr(logits2d), ptr(target), ptr(lse), ptr(grad_scale), ptr(dlogits), rows, V, ld,
               ignore_index, dtype_code(logits2d), stream())
    return dlogits


def ls_cross_entropy_fwd(logits2d, target, V, ignore_index, eps, cstart=-1, cend=-1, cmask=None):
    """label-smoothed CE rows: returns lse, row_loss, row_nll, row_cnt (fp32 [rows])."""
    rows, ld = logits2d.shape[0], logits2d.stride(0)
    out = [torch.empty(rows, dtype=torch.float32, device=logits2d.device) for _ in range(4)]
    if cmask is not None:
        cmask = _u8(cmask)
    lib().call("ofa_ls_cross_entropy_fwd", ptr(logits2d), ptr(target), *[ptr(o) for o in out], rows, V, ld, ignore_index,
               float(eps), int(cstart), int(cend), ptr(cmask), dtype_code(logits2d), stream())
    return out


def ls_cross_entropy_bwd(logits2d, target, lse, row_cnt, row_w, grad_scale, V, ignore_index, eps, cstart=-1, cend=-1,
                         cmask=None):
    rows, ld = logits2d.shape[0], logits2d.stride(0)
    dlogits = torch.empty(rows, ld, dtype=logits2d.dtype, device=logits2d.device)
    if cmask is not None:
        cmask = _u8(cmask)
    lib().call("ofa_ls_cross_entropy_bwd", ptr(logits2d), ptr(target), ptr(lse), ptr(row_cnt), ptr(row_w), ptr(grad_scale),
               ptr(dlogits), rows, V, ld, ignore_index, float(eps), int(cstart), int(cend), ptr(cmask),
               dtype_code(logits2d), stream())
    return dlogits


def _trie_args(logits2d, target, nodes, trie):
    """The checked (node, node_edge_off, edge_token, N, E) arguments of ofa_trie_ls_cross_entropy_*; trie: a dict with the int32 device
    arrays "node_edge_off" [N + 1], "edge_token" [E] and the ints "N", "E" (traverse.TraversePlan.to_device)."""
    rows = logits2d.shape[0]
    off, tok, N, E = trie["node_edge_off"], trie["edge_token"], int(trie["N"]), int(trie["E"])
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == rows, (target.dtype, target.shape, rows)
    assert nodes.dtype == torch.int32 and nodes.is_contiguous() and nodes.numel() == rows, (nodes.dtype, nodes.shape, rows)
    assert off.dtype == torch.int32 and off.is_contiguous() and off.numel() == N + 1, (off.dtype, off.shape, N)
    assert tok.dtype == torch.int32 and tok.is_contiguous() and tok.numel() == E, (tok.dtype, tok.shape, E)
    return ptr(nodes), ptr(off), ptr(tok), N, E


def trie_ls_cross_entropy_fwd(logits2d, target, nodes, trie, V, ignore_index, eps, cstart=-1, cend=-1, grad_scale=None, want_grad=False):
    """Label-smoothed CE rows whose allowed set is the children of the trie node nodes[row] (ofa_trie_ls_cross_entropy_fwd): returns
    lse, row_loss, row_nll, row_cnt (fp32 [rows]) and, with want_grad, dlogits [rows, ld] at grad_scale[0] (fp32 device scalar, None: 1)
    written by the same launch (else None)."""
    rows, ld = logits2d.shape[0], logits2d.stride(0)
    targs = _trie_args(logits2d, target, nodes, trie)
    out = [torch.empty(rows, dtype=torch.float32, device=logits2d.device) for _ in range(4)]
    dlogits = torch.empty(rows, ld, dtype=logits2d.dtype, device=logits2d.device) if want_grad else None
    lib().call("ofa_trie_ls_cross_entropy_fwd", ptr(logits2d), ptr(target), *targs, ptr(grad_scale), *[ptr(o) for o in out],
               ptr(dlogits), rows, V, ld, ignore_index, float(eps), int(cstart), int(cend), dtype_code(logits2d), stream())
    return (*out, dlogits)


def trie_ls_cross_entropy_bwd(logits2d, target, nodes, trie, lse, row_cnt, row_w, grad_scale, V, ignore_index, eps, cstart=-1, cend=-1,
                              dlogits=None):
    """dlogits [rows, ld] at grad_scale[0] * row_w[row] from the forward's lse and row_cnt (ofa_trie_ls_cross_entropy_bwd)."""
    rows, ld = logits2d.shape[0], logits2d.stride(0)
    targs = _trie_args(logits2d, target, nodes, trie)
    if dlogits is None:
        dlogits = torch.empty(rows, ld, dtype=logits2d.dtype, device=logits2d.device)
    lib().call("ofa_trie_ls_cross_entropy_bwd", ptr(logits2d), ptr(target), *targs, ptr(lse), ptr(row_cnt), ptr(row_w), ptr(grad_scale),
               ptr(dlogits), rows, V, ld, ignore_index, float(eps), int(cstart), int(cend), dtype_code(logits2d), stream())
    return dlogits


# ------------------------------------------------------------------ trie-edge head (csrc/trie_head.hip)
HEAD_TRIE_KEYS = ("node_edge_off", "edge_token", "edge_node", "head_tokens", "tok_edge_off", "tok_edge")


def _trie_head_proj(who, feats, weight, bias):
    if feats.dim() != 2 or weight.dim() != 2 or feats.stride(1) != 1 or weight.stride(1) != 1:
        raise OfaError(f"{who}: features [rows, D] and projection rows [V, D] must have a contiguous last dimension")
    if weight.dtype != feats.dtype or (bias is not None and bias.dtype != feats.dtype):
        raise OfaError(f"{who}: features ({feats.dtype}), projection ({weight.dtype}) and bias must share one dtype")
    if weight.shape[1] != feats.shape[1] or (bias is not None and (bias.numel() != weight.shape[0] or not bias.is_contiguous())):
        raise OfaError(f"{who}: projection [V, D] / bias [V] do not match the features' width")


def _ld(x):
    return x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1])


def trie_head_cmax(trie):
    """The slots per row of the trie-edge head's compact buffers: the plan's max_degree, which the trie dict must carry."""
    if trie.get("max_degree") is None:
        raise ValueError("trie_head: the trie's device arrays carry no \"max_degree\" (TraversePlan.head_arrays / to_device do)")
    return int(trie["max_degree"])


def trie_head_fwd(feats, weight, bias, target, nodes, trie, ignore_index, eps, cstart=-1, cend=-1, want_grad=True, want_hit=False):
    """The trie-edge head's forward launch (ofa_trie_head_fwd): feats [rows, D], weight [V, D], bias [V] or None of one dtype; target
    int64 [rows], nodes int32 [rows]; trie: the device arrays of TraversePlan.head_arrays.  -> dict(z, g fp32 [rows, Cmax] (g None
    without want_grad), lse, row_loss, row_nll, row_cnt fp32 [rows], row_hit int32 [rows] or None).  Slots past a row's degree are
    not written."""
    _trie_head_proj("trie_head_fwd", feats, weight, bias)
    rows, D = feats.shape
    V = weight.shape[0]
    targs = _trie_args(feats, target, nodes, trie)
    Cmax = trie_head_cmax(trie)
    dev = feats.device
    z = torch.empty(rows, Cmax, dtype=torch.float32, device=dev)
    g = torch.empty(rows, Cmax, dtype=torch.float32, device=dev) if want_grad else None
    out = [torch.empty(rows, dtype=torch.float32, device=dev) for _ in range(4)]
    hit = torch.empty(rows, dtype=torch.int32, device=dev) if want_hit else None
    lib().call("ofa_trie_head_fwd", ptr(feats), _ld(feats), ptr(weight), _ld(weight), ptr(bias), D, V, ptr(target), *targs, Cmax, ptr(z),
               *[ptr(o) for o in out], ptr(g), ptr(hit), rows, int(ignore_index), float(eps), int(cstart), int(cend), dtype_code(feats),
               stream())
    return dict(z=z, g=g, lse=out[0], row_loss=out[1], row_nll=out[2], row_cnt=out[3], row_hit=hit)


def trie_head_bwd_dx(g, weight, target, nodes, trie, row_w, grad_scale, ignore_index, cstart=-1, cend=-1, out=None):
    """dfeats [rows, D] of weight's dtype = grad_scale[0] * row_w[r] * sum_j g[r, j] W[tok_j] (ofa_trie_head_bwd_dx); every row is
    written.  row_w fp32 [rows] and grad_scale (fp32 device scalar) are optional."""
    rows, D = g.shape[0], weight.shape[1]
    targs = _trie_args(g, target, nodes, trie)
    Cmax = trie_head_cmax(trie)
    assert g.dtype == torch.float32 and g.is_contiguous() and g.shape == (rows, Cmax), (g.dtype, g.shape, Cmax)
    if out is None:
        out = torch.empty(rows, D, dtype=weight.dtype, device=weight.device)
    lib().call("ofa_trie_head_bwd_dx", ptr(g), ptr(weight), _ld(weight), D, weight.shape[0], ptr(target), *targs, Cmax, ptr(row_w),
               ptr(grad_scale), ptr(out), _ld(out), rows, int(ignore_index), int(cstart), int(cend), dtype_code(weight), stream())
    return out


def trie_head_buckets(nodes, trie):
    """The step's row buckets, on the device without a host synchronisation: (bucket_rows int32 [rows]: the row indices ordered by node,
    ascending within a node; bucket_off int32 [N + 1]).  Rows on a node outside [0, N) sort past every bucket."""
    N = int(trie["N"])
    nd = nodes.reshape(-1)
    key = torch.where((nd >= 0) & (nd < N), nd, torch.full_like(nd, N))
    skey, order = torch.sort(key, stable=True)
    ids = trie.get("node_ids")
    if ids is None:
        ids = torch.arange(N + 1, dtype=torch.int32, device=nd.device)
    off = torch.searchsorted(skey, ids, out_int32=True)
    return order.to(torch.int32), off


def trie_head_bwd_dw(g, feats, trie, buckets, row_w, grad_scale, dweight, dbias=None, cstart=-1, cend=-1):
    """dweight[u] += grad_scale[0] * sum over (row, slot) pairs whose token is u of row_w[r] g[r, slot] feats[r] (ofa_trie_head_bwd_dw),
    dbias[u] likewise: a PARTIAL writer of dweight -- it touches the rows of the tokens that have contributing rows and nothing
    else -- in a fixed order, without float atomics.  buckets: trie_head_buckets(nodes, trie) of this step."""
    rows, D = feats.shape
    Cmax = trie_head_cmax(trie)
    N, E, U = int(trie["N"]), int(trie["E"]), int(trie["U"])
    for k in HEAD_TRIE_KEYS:
        assert trie[k].dtype == torch.int32 and trie[k].is_contiguous(), k
    assert trie["head_tokens"].numel() == U and trie["tok_edge_off"].numel() == U + 1 and trie["tok_edge"].numel() == E
    assert trie["edge_node"].numel() == E and trie["node_edge_off"].numel() == N + 1
    brows, boff = buckets
    assert brows.dtype == boff.dtype == torch.int32 and brows.numel() == rows and boff.numel() == N + 1
    assert g.dtype == torch.float32 and g.is_contiguous() and g.shape == (rows, Cmax), (g.dtype, g.shape, Cmax)
    assert dweight.dtype == feats.dtype and dweight.stride(1) == 1 and dweight.shape[1] == D and feats.stride(1) == 1
    assert dbias is None or (dbias.dtype == feats.dtype and dbias.is_contiguous() and dbias.numel() == dweight.shape[0])
    _accum(dweight, True, full=False)                # the rows of the batch's tokens only: a partial writer always adds
    if dbias is not None:
        _accum(dbias, True, full=False)
    lib().call("ofa_trie_head_bwd_dw", ptr(g), ptr(feats), _ld(feats), D, dweight.shape[0], ptr(trie["node_edge_off"]),
               ptr(trie["edge_node"]), N, E, Cmax, ptr(trie["head_tokens"]), ptr(trie["tok_edge_off"]), ptr(trie["tok_edge"]), U,
               ptr(brows), ptr(boff), ptr(row_w), ptr(grad_scale), ptr(dweight), _ld(dweight), ptr(dbias), rows, int(cstart), int(cend),
               dtype_code(feats), stream())
    return dweight


def criterion_eval(logits2d, target, V, ignore_index, eps, cstart=-1, cend=-1, cmask=None, nodes=None, trie=None):
    """Validation's criterion rows in one read of the logits (ofa_criterion_eval): returns row_loss, row_nll (fp32 [rows]) and row_hit
    (int32 [rows]: the target is the arg-max over the allowed set).  The allowed set: the whole vocabulary, the range, a byte mask
    [rows, V], or the children of trie node nodes[row] (`trie` as in trie_ls_cross_entropy_fwd).  The outputs are fresh tensors (inside
    a capture: of the capturing graph's pool), there is no other scratch."""
    rows, ld = logits2d.shape[0], logits2d.stride(0) if logits2d.shape[0] > 1 else max(logits2d.stride(0), V)
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == rows, (target.dtype, target.shape, rows)
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits2d.device)
    row_nll = torch.empty(rows, dtype=torch.float32, device=logits2d.device)
    row_hit = torch.empty(rows, dtype=torch.int32, device=logits2d.device)
    targs = (None, None, None, 0, 0)
    if nodes is not None:
        if trie is None:
            raise ValueError("criterion_eval: nodes need the trie's device arrays")
        targs = _trie_args(logits2d, target, nodes, trie)
    if cmask is not None:
        cmask = _u8(cmask)
        assert cmask.is_contiguous() and cmask.numel() == rows * V, (cmask.shape, rows, V)
    lib().call("ofa_criterion_eval", ptr(logits2d), ptr(target), ptr(cmask), *targs, ptr(row_loss), ptr(row_nll), ptr(row_hit), rows, V, ld,
               int(ignore_index), float(eps), int(cstart), int(cend), dtype_code(logits2d), stream())
    return row_loss, row_nll, row_hit


def eval_stats_add(acc, row_loss, row_nll, row_hit, target, ignore_index):
    """acc (fp64 [4]: ntokens, loss_sum, nll_sum, n_correct) += one batch's rows, summed in a fixed order by one block
    (ofa_eval_stats_add): the same inputs give the same bits."""
    assert acc.dtype == torch.float64 and acc.numel() >= 4 and acc.is_contiguous()
    rows = row_loss.numel()
    t = target.reshape(-1)
    assert t.dtype == torch.int64 and t.is_contiguous() and t.numel() == rows
    assert row_loss.dtype == row_nll.dtype == torch.float32 and row_hit.dtype == torch.int32 and row_nll.numel() == row_hit.numel() == rows
    lib().call("ofa_eval_stats_add", ptr(acc), ptr(row_loss), ptr(row_nll), ptr(row_hit), ptr(t), rows, int(ignore_index), stream())


def scst_loss_fwd_grad(logits2d, target, reward, grad_scale, V, ignore_index, rows_per_seq=1, row_seq=None, cstart=-1, cend=-1,
                       dlogits=None):
    """Reward-weighted NLL rows and their gradient in one call (ofa_scst_loss_fwd_grad): returns lse, row_loss (fp32 [rows]) and
    dlogits [rows, ld] = reward[sentence] * grad_scale[0] * (softmax - onehot) over the allowed vocabulary.  reward: fp32 [nseq];
    the sentence of row r is row_seq[r] (int32 [rows]) or r // rows_per_seq; grad_scale: fp32 device scalar (None: 1)."""
    rows, ld = logits2d.shape[0], logits2d.stride(0)
    assert reward.dtype == torch.float32 and reward.is_contiguous() and target.dtype == torch.int64 and target.is_contiguous()
    assert target.numel() == rows, (target.shape, rows)
    if row_seq is not None:
        assert row_seq.dtype == torch.int32 and row_seq.is_contiguous() and row_seq.numel() == rows, (row_seq.dtype, row_seq.shape)
    else:
        assert rows <= reward.numel() * int(rows_per_seq), (rows, reward.numel(), rows_per_seq)
    lse = torch.empty(rows, dtype=torch.float32, device=logits2d.device)
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits2d.device)
    if dlogits is None:
        dlogits = torch.empty(rows, ld, dtype=logits2d.dtype, device=logits2d.device)
    lib().call("ofa_scst_loss_fwd_grad", ptr(logits2d), ptr(target), ptr(reward), ptr(row_seq), int(rows_per_seq), ptr(grad_scale),
               ptr(lse), ptr(row_loss), ptr(dlogits), rows, reward.numel(), V, ld, ignore_index, int(cstart), int(cend),
               dtype_code(logits2d), stream())
    return lse, row_loss, dlogits


def probs_fwd(logits2d, V, ld, log_probs):
    rows = logits2d.shape[0]
    y = torch.empty(rows, V, dtype=torch.float32, device=logits2d.device)
    lib().call("ofa_probs_fwd", ptr(logits2d), ptr(y), rows, V, ld, int(log_probs), dtype_code(logits2d), stream())
    return y


def probs_bwd(dy, y, V, dtype, log_probs):
    rows = y.shape[0]
    ld = (V + 7) // 8 * 8
    d = torch.empty(rows, ld, dtype=dtype, device=y.device)
    lib().call("ofa_probs_bwd", ptr(dy), ptr(y), ptr(d), rows, V, ld, int(log_probs), dtype_code(d), stream())
    return d


def sumsq(x, out):
    """out (fp32[1]) += sum(x*x)."""
    x = x.contiguous()
    ws = workspace(lib().cdll.ofa_sumsq_ws_floats() * 4, x.device, "sumsq")
    lib().call("ofa_sumsq", ptr(x), ptr(out), ptr(ws), x.numel(), dtype_code(x), stream())
    return out


def sumsq_schedule(x, gsq, ticket, sample_size, step, lr, sched, gnorm, clip_norm, beta1, beta2, loss_scaler=None, scale_factor=2.0,
                   scale_window=2000, tolerance=0.0, threshold=None, min_loss_scale=1e-4, counter=None, counter_add=0):
    """sumsq(x) -> gsq (written), then step_schedule / step_schedule_scaled (loss_scaler given) and counter += counter_add (an int64
    device scalar, optional), all in ONE launch (ofa_sumsq_schedule): the same bits as the separate launches.  ticket: one int32 device
    word, 0 before the first call (the kernel resets it)."""
    assert x.is_contiguous() and x.numel() >= 1 and ticket.dtype == torch.int32 and (counter is None or counter.dtype == torch.int64)
    ws = workspace(lib().cdll.ofa_sumsq_ws_floats() * 4, x.device, "sumsq")
    lib().call("ofa_sumsq_schedule", ptr(x), ptr(gsq), ptr(ws), ptr(ticket), x.numel(), dtype_code(x), ptr(sample_size), ptr(step),
               ptr(lr), ptr(sched), ptr(gnorm), ptr(loss_scaler), ptr(counter), int(counter_add), float(clip_norm), float(beta1),
               float(beta2), float(scale_factor), float(scale_window), float(tolerance), float(threshold or 0.0), float(min_loss_scale),
               stream())


def step_schedule(gsq, sample_size, step, lr, sched, gnorm, clip_norm, beta1, beta2):
    """Device-side scalar schedule of one update (see ofa_step_schedule); all arguments are 1-element device tensors
    (gsq fp32, sample_size / step / lr fp64, sched fp32[3], gnorm fp32)."""
    lib().call("ofa_step_schedule", ptr(gsq), ptr(sample_size), ptr(step), ptr(lr), ptr(sched), ptr(gnorm), float(clip_norm),
               float(beta1), float(beta2), stream())


def step_schedule_scaled(gsq, sample_size, step, lr, sched, gnorm, loss_scaler, clip_norm, beta1, beta2, scale_factor=2.0,
                         scale_window=2000, tolerance=0.0, threshold=None, min_loss_scale=1e-4):
    """step_schedule with the reference's dynamic loss scaler (see ofa_step_schedule_scaled); loss_scaler: fp64[8] device state."""
    lib().call("ofa_step_schedule_scaled", ptr(gsq), ptr(sample_size), ptr(step), ptr(lr), ptr(sched), ptr(gnorm), ptr(loss_scaler),
               float(clip_norm), float(beta1), float(beta2), float(scale_factor), float(scale_window), float(tolerance),
               float(threshold or 0.0), float(min_loss_scale), stream())


def adam_step(master, exp_avg, exp_avg_sq, grad, model_param, coef, lr, beta1, beta2, eps, weight_decay, step, max_blocks=0):
    """max_blocks > 0: ofa_adam_step_grid with the grid capped there (a test reaches the second quad and the second trip at a small n)."""
    args = (ptr(master), ptr(exp_avg), ptr(exp_avg_sq), ptr(grad), ptr(model_param), ptr(coef), master.numel(), float(lr), float(beta1),
            float(beta2), float(eps), float(weight_decay), int(step), dtype_code(grad))
    if max_blocks:
        lib().call("ofa_adam_step_grid", *args, int(max_blocks), stream())
    else:
        lib().call("ofa_adam_step", *args, stream())


class _EmaSegment(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("off", ctypes.c_int64), ("len", ctypes.c_int64)]


def ema_step(state, p, shadow, step, sched, decay, start_update=0, update_freq=1, max_blocks=0):
    """One EMA update of a flat arena, decided on the device (ofa_ema_step): state (fp32, or p's dtype) <- d * state + (1 - d) * p
    when sched[3] == 0 and step[0] % update_freq == 0, d = 0 before start_update; shadow (None, or p's dtype): round(state)."""
    assert state.is_contiguous() and p.is_contiguous() and state.numel() == p.numel() and step.dtype == torch.float64
    assert shadow is None or (shadow.is_contiguous() and shadow.dtype == p.dtype and shadow.numel() == p.numel())
    lib().call("ofa_ema_step", ptr(state), ptr(p), ptr(shadow), p.numel(), ptr(step), ptr(sched), float(decay), int(start_update),
               int(update_freq), dtype_code(p), dtype_code(state), int(max_blocks), stream())


def ema_segment_table(sources, offsets, device):
    """The device table of ofa_ema_segments_step: (source tensor, offset into the state array) per floating-point tensor outside
    the arena.  Returns (table, longest length); the caller keeps the sources alive for as long as it uses the table."""
    arr = (_EmaSegment * max(len(sources), 1))()
    for it, s, o in zip(arr, sources, offsets):
        assert s.is_contiguous()
        it.src, it.off, it.len = dptr(s), int(o), s.numel()
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.int64).clone()
    return raw.to(device), max([s.numel() for s in sources], default=0)


def ema_segments_step(state, table, nseg, max_len, shadow, model_dtype, step, sched, decay, start_update=0, update_freq=1,
                      max_blocks=0):
    """ema_step for every segment of `table` (ema_segment_table) in one launch; the sources (and `shadow`) are of `model_dtype`."""
    code = dtype_code(torch.empty(0, dtype=model_dtype))
    assert state.is_contiguous() and step.dtype == torch.float64 and table.dtype == torch.int64 and table.numel() >= 3 * nseg
    assert shadow is None or (shadow.is_contiguous() and shadow.numel() == state.numel() and shadow.dtype == model_dtype)
    lib().call("ofa_ema_segments_step", ptr(state), ptr(table), ptr(shadow), int(nseg), state.numel(), int(max_len), ptr(step),
               ptr(sched), float(decay), int(start_update), int(update_freq), code, dtype_code(state), int(max_blocks), stream())


def colsum(x, alpha=1.0, out=None, accumulate=False, out_dtype=torch.float32, fold=None, same_bits=False):
    """Column sums of a 2-D tensor (last dim contiguous): fresh tensor of `out_dtype`, or (accumulated) into `out`.
    fold (with out): only the row-group partials are computed now, the FoldQueue finishes the sum at its flush.  same_bits: the queue
    adds the partials in the order of the immediate final pass (for the callers that used to finish the sum themselves); without it
    a sum over more than 1024 rows is grouped as the queue's LayerNorm jobs are."""
    if x.stride(-1) != 1:
        x = x.contiguous()
    rows, cols = x.shape
    if out is None:
        out = torch.empty(cols, dtype=out_dtype, device=x.device)
        fold = None
    if fold is not None and out.is_contiguous():
        ns = lib().cdll.ofa_colsum_slots(rows)
        ws = torch.empty(ns * cols, dtype=torch.float32, device=x.device)
        fold.add(ws, 0, out, cols, cols, ns, alpha, accumulate, lanes16=same_bits)
        lib().call("ofa_colsum", ptr(x), ptr(out), ptr(ws), rows, cols, x.stride(0), float(alpha), DEFER_FOLD,
                   dtype_code(x), dtype_code(out), stream())
        fold.flush_if_large()
        return out
    ws = workspace(lib().cdll.ofa_colsum_ws_floats(cols) * 4, x.device, "colsum")
    lib().call("ofa_colsum", ptr(x), ptr(out), ptr(ws), rows, cols, x.stride(0), float(alpha),
               int(_accum(out, accumulate, full=out.is_contiguous())), dtype_code(x), dtype_code(out), stream())
    return out


def mul(a, b):
    a, b = a.contiguous(), b.contiguous()
    rows, cols = _rows_cols(a)
    y = torch.empty_like(a)
    lib().call("ofa_mul", ptr(a), ptr(b), ptr(y), rows, cols, 0, dtype_code(a), stream())
    return y


def add_n(tensors):
    """sum of up to 16 same-shaped tensors in one launch (fp32 accumulation, one rounding)."""
    ts = [t.contiguous() for t in tensors]
    assert 1 <= len(ts) <= 16 and all(t.shape == ts[0].shape and t.dtype == ts[0].dtype for t in ts)
    if len(ts) == 1:
        return ts[0]
    out = torch.empty_like(ts[0])
    arr = (ctypes.c_void_p * len(ts))(*[dptr(t) for t in ts])
    lib().call("ofa_add_n", ctypes.addressof(arr), len(ts), ptr(out), out.numel(), dtype_code(out), stream())
    return out


def mul_rowvec(a, vec):
    a, vec = a.contiguous(), vec.contiguous()
    rows, cols = _rows_cols(a)
    y = torch.empty_like(a)
    lib().call("ofa_mul", ptr(a), ptr(vec), ptr(y), rows, cols, 1, dtype_code(a), stream())
    return y


def scale_row_groups(x, scale, group):
    """y[r, :] = x[r, :] * scale[r // group]; x: [rows, cols] rows, scale: fp32 [rows // group]."""
    x = x.contiguous()
    rows, cols = _rows_cols(x)
    assert scale.dtype == torch.float32 and scale.numel() * group == rows
    y = torch.empty_like(x)
    lib().call("ofa_scale_row_groups", ptr(x), ptr(scale.contiguous()), ptr(y), rows, cols, group, dtype_code(x), stream())
    return y


def sum_f32(x):
    x = x.contiguous()
    out = torch.empty((), dtype=torch.float32, device=x.device)
    lib().call("ofa_reduce_sum_f32", ptr(x), ptr(out), x.numel(), stream())
    return out


def bias_block_add_(bias, values, start):
    """In place: bias[B,A,T,T][:, :, s:s+n, s:s+n] += values[n,n,A] (broadcast over batch)."""
    B, A, T, _ = bias.shape
    n = values.shape[0]
    values = values.contiguous()
    assert bias.is_contiguous() and values.dtype == bias.dtype
    lib().call("ofa_bias_block_add", ptr(bias), ptr(values), B, A, T, start, n, dtype_code(bias), stream())
    return bias


def bias_block_add_batch_(bias, values, start):
    """In place: bias[B,A,T,T][:, :, s:s+n, s:s+n] += values[B,A,n,n] (one matrix per sample and head)."""
    B, A, T, _ = bias.shape
    n = values.shape[-1]
    values = values.contiguous()
    assert bias.is_contiguous() and values.dtype == bias.dtype and tuple(values.shape) == (B, A, n, n)
    lib().call("ofa_bias_block_add_batch", ptr(bias), ptr(values), B, A, T, start, n, dtype_code(bias), stream())
    return bias


def bias_block_slice(dbias, start, n):
    """dbias[B,A,T,T][:, :, s:s+n, s:s+n] as a contiguous [B,A,n,n] tensor (the gradient of bias_block_add_batch_'s values)."""
    dbias = dbias.contiguous()
    B, A, T, _ = dbias.shape
    out = torch.empty(B, A, n, n, dtype=dbias.dtype, device=dbias.device)
    lib().call("ofa_bias_block_slice", ptr(dbias), ptr(out), B, A, T, start, n, dtype_code(dbias), stream())
    return out


def bias_outer_grad(dbias, start, F, P):
    """dbias [1|.., A, T, T] (one matrix) -> (d_frames [F,F,A], d_patches [P,P,A]) of an OUTER slot at `start` (ofa_bias_outer_grad)."""
    dbias = dbias.contiguous()
    A, T = dbias.shape[-3], dbias.shape[-1]
    assert dbias.numel() == A * T * T
    dvf = torch.empty(F, F, A, dtype=dbias.dtype, device=dbias.device)
    dvi = torch.empty(P, P, A, dtype=dbias.dtype, device=dbias.device)
    lib().call("ofa_bias_outer_grad", ptr(dbias), ptr(dvf), ptr(dvi), A, T, start, F, P, dtype_code(dbias), stream())
    return dvf, dvi


def bias_block_grad(dbias, start, n):
    dbias = dbias.contiguous()
    B, A, T, _ = dbias.shape
    dvalues = torch.empty(n, n, A, dtype=dbias.dtype, device=dbias.device)
    lib().call("ofa_bias_block_grad", ptr(dbias), ptr(dvalues), B, A, T, start, n, dtype_code(dbias), stream())
    return dvalues


def mean_heads(p, B, heads):
    """p: [B*heads, T, S] -> [B, T, S] mean over heads."""
    p = p.contiguous()
    T, S = p.shape[1], p.shape[2]
    out = torch.empty(B, T, S, dtype=p.dtype, device=p.device)
    lib().call("ofa_mean_heads", ptr(p), ptr(out), B, heads, T * S, dtype_code(p), stream())
    return out


def head_sum(x, B, heads, T):
    """x: fp32 [B*heads, ld] -> [heads] sums over batch and the first T columns."""
    out = torch.empty(heads, dtype=torch.float32, device=x.device)
    lib().call("ofa_head_sum_f32", ptr(x), ptr(out), B, heads, T, x.stride(0), stream())
    return out


# ------------------------------------------------------------------ convolution stack (NHWC rows), csrc/conv.hip
def conv_out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def im2col(x, B, H, W, C, kh, kw, stride, pad, nchw=False):
    """x: NHWC rows [B*H*W, C] (or the [B,C,H,W] image when nchw) -> col [B*Ho*Wo, Kpad], taps ordered (kh, kw, c)."""
    x = x.contiguous()
    Ho, Wo = conv_out_size(H, kh, stride, pad), conv_out_size(W, kw, stride, pad)
    K = kh * kw * C
    Kpad = (K + 7) // 8 * 8
    col = torch.empty(B * Ho * Wo, Kpad, dtype=x.dtype, device=x.device)
    lib().call("ofa_im2col", ptr(x), ptr(col), B, H, W, C, kh, kw, stride, pad, Kpad, int(nchw), dtype_code(x), stream())
    return col, Ho, Wo


def col2im(dcol, B, H, W, C, kh, kw, stride, pad):
    dcol = dcol.contiguous()
    dx = torch.empty(B * H * W, C, dtype=dcol.dtype, device=dcol.device)
    lib().call("ofa_col2im", ptr(dcol), ptr(dx), B, H, W, C, kh, kw, stride, pad, dcol.shape[1], dtype_code(dcol), stream())
    return dx


def batchnorm_fwd(x, gamma, beta, running_mean, running_var, training, momentum, eps, relu=False, residual=None):
    """x: [rows, C].  Returns y, mean, rstd (fp32 [C]); updates the running buffers in training mode."""
    x = x.contiguous()
    rows, C = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = workspace(lib().cdll.ofa_batchnorm_ws_floats(C) * 4, x.device, "bn")
    if residual is not None:
        residual = residual.contiguous()
    lib().call("ofa_batchnorm_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(residual), ptr(y), ptr(mean), ptr(rstd),
               ptr(running_mean), ptr(running_var), ptr(ws), rows, C, float(eps), float(momentum), int(not training),
               int(relu), dtype_code(x), stream())
    return y, mean, rstd


def batchnorm_bwd(dy, y, x, gamma, mean, rstd, batch_stats, relu, want_dres=False, dgamma=None, dbeta=None, beta=None):
    """beta (relu layers without a residual only): the ReLU gate is recomputed from x instead of read from y."""
    dy = dy.contiguous()
    rows, C = x.shape
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    acc = dgamma is not None
    if not acc:
        dgamma = torch.empty(C, dtype=gamma.dtype, device=x.device)
        dbeta = torch.empty(C, dtype=gamma.dtype, device=x.device)
    ws = workspace(lib().cdll.ofa_batchnorm_ws_floats(C) * 4, x.device, "bn")
    if acc:
        acc = _accum_all([dgamma, dbeta])
    lib().call("ofa_batchnorm_bwd", ptr(dy), ptr(y), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dres), ptr(dgamma),
               ptr(dbeta), ptr(ws), rows, C, int(batch_stats), int(relu), int(acc), ptr(beta) if (relu and not want_dres) else None,
               dtype_code(x), stream())
    return dx, dres, dgamma, dbeta


def batchnorm_fwd_stats(x):
    """SyncBatchNorm, forward phase 1: this rank's [2*C + 1] fp64 sums (sum x, sum x^2, row count) -- to be all-reduced."""
    x = x.contiguous()
    rows, C = x.shape
    sums = torch.empty(2 * C + 1, dtype=torch.float64, device=x.device)
    ws = workspace(lib().cdll.ofa_batchnorm_ws_floats(C) * 4, x.device, "bn")
    lib().call("ofa_batchnorm_fwd_stats", ptr(x), ptr(sums), ptr(ws), rows, C, dtype_code(x), stream())
    return sums


def batchnorm_fwd_apply(x, gamma, beta, running_mean, running_var, sums, momentum, eps, relu=False, residual=None, groups=0):
    """Forward from statistics that exist already; returns y, mean, rstd.  groups = 0: SyncBatchNorm phase 2 (`sums` = the
    all-reduced [2C + 1] sums); groups > 0: `sums` = [groups, 2, C] partial rows over x's rows (a convolution's GEMM epilogue)."""
    x = x.contiguous()
    rows, C = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(C, dtype=torch.float32, device=x.device)
    if residual is not None:
        residual = residual.contiguous()
    lib().call("ofa_batchnorm_fwd_apply", ptr(x), ptr(gamma), ptr(beta), ptr(residual), ptr(y), ptr(mean), ptr(rstd),
               ptr(running_mean), ptr(running_var), ptr(sums), int(groups), rows, C, float(eps), float(momentum), int(relu),
               dtype_code(x), stream())
    return y, mean, rstd


def batchnorm_bwd_stats(dy, y, x, gamma, mean, rstd, relu, regate_beta=None, dgamma=None, dbeta=None):
    """SyncBatchNorm, backward phase 1: this rank's [2, C] fp32 sums (sum g, sum g*xhat) -- to be all-reduced -- and the rank-local
    parameter gradients (accumulated into dgamma / dbeta when given)."""
    dy = dy.contiguous()
    rows, C = x.shape
    acc = dgamma is not None
    if not acc:
        dgamma = torch.empty(C, dtype=gamma.dtype, device=x.device)
        dbeta = torch.empty(C, dtype=gamma.dtype, device=x.device)
    sums = torch.empty(2, C, dtype=torch.float32, device=x.device)
    ws = workspace(lib().cdll.ofa_batchnorm_ws_floats(C) * 4, x.device, "bn")
    if acc:
        acc = _accum_all([dgamma, dbeta])
    lib().call("ofa_batchnorm_bwd_stats", ptr(dy), ptr(y), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(sums), ptr(dgamma), ptr(dbeta),
               ptr(ws), rows, C, int(relu), int(acc), ptr(regate_beta), dtype_code(x), stream())
    return sums, dgamma, dbeta


def batchnorm_bwd_dx(dy, y, x, gamma, mean, rstd, sums, total_rows, relu, want_dres=False, regate_beta=None):
    """SyncBatchNorm, backward phase 2 (sums all-reduced; total_rows: 1-element fp64 device tensor)."""
    dy = dy.contiguous()
    rows, C = x.shape
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    assert total_rows.dtype == torch.float64 and total_rows.numel() == 1
    lib().call("ofa_batchnorm_bwd_dx", ptr(dy), ptr(y), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(sums), ptr(dx), ptr(dres), rows,
               ptr(total_rows), C, int(relu), ptr(regate_beta), dtype_code(x), stream())
    return dx, dres


def maxpool_fwd(x, B, H, W, C, k, stride, pad):
    x = x.contiguous()
    Ho, Wo = conv_out_size(H, k, stride, pad), conv_out_size(W, k, stride, pad)
    y = torch.empty(B * Ho * Wo, C, dtype=x.dtype, device=x.device)
    arg = torch.empty(B * Ho * Wo, C, dtype=torch.uint8, device=x.device)
    lib().call("ofa_maxpool_fwd", ptr(x), ptr(y), ptr(arg), B, H, W, C, k, stride, pad, dtype_code(x), stream())
    return y, arg, Ho, Wo


def maxpool_bwd(dy, arg, B, H, W, C, k, stride, pad):
    dy = dy.contiguous()
    dx = torch.empty(B * H * W, C, dtype=dy.dtype, device=dy.device)
    lib().call("ofa_maxpool_bwd", ptr(dy), ptr(arg), ptr(dx), B, H, W, C, k, stride, pad, dtype_code(dy), stream())
    return dx


def relu(x, gate=None):
    x = x.contiguous()
    y = torch.empty_like(x)
    lib().call("ofa_relu", ptr(x), ptr(gate), ptr(y), x.numel(), dtype_code(x), stream())
    return y


# ------------------------------------------------------------------ residual join (csrc/join.hip)
def join_fwd(x, residual, ln_a, ln_b, eps, p, seed, offset, offset_base):
    """y = residual + dropout_p(LN_a(x)); z = LN_b(y).  ln_a / ln_b: (gamma, beta) or None.  Returns y, z (or None), stats, keep_bits
    (the dropout decisions for join_bwd, or None: this shape regenerates them)."""
    x = x.contiguous()
    residual = residual.contiguous() if residual is not None else None       # None: y = dropout_p(LN_a(x))
    rows, cols = _rows_cols(x)
    y = torch.empty_like(x)
    z = torch.empty_like(x) if ln_b is not None else None
    stats = torch.empty(4, rows, dtype=torch.float32, device=x.device)
    nkeep = lib().cdll.ofa_join_keep_bytes(rows, cols, dtype_code(x)) if p > 0 else 0
    keep = torch.empty(nkeep, dtype=torch.uint8, device=x.device) if nkeep else None
    ga, ba = ln_a if ln_a is not None else (None, None)
    gb, bb = ln_b if ln_b is not None else (None, None)
    lib().call("ofa_join_fwd", ptr(x), ptr(residual), ptr(ga), ptr(ba), ptr(gb), ptr(bb), ptr(y), ptr(z), ptr(stats), ptr(keep), rows, cols,
               float(eps), float(p), seed, offset, ptr(offset_base), dtype_code(x), stream())
    return y, z, stats, keep


def join_bwd(dy, dz, x, y, ga, gb, stats, p, seed, offset, offset_base, grads, fold=None, want_dres=True, keep=None):
    """grads = (dgamma_a, dbeta_a, dgamma_b, dbeta_b[, dx_colsum]) output tensors (accumulated into; None for an absent
    LayerNorm; dx_colsum: the bias gradient of the Linear that produced x, optional).
    Returns dres, dx.  The column partials are folded by `fold` (a FoldQueue) or immediately."""
    like = dy if dy is not None else dz
    rows, cols = _rows_cols(like)
    dres, dx = (torch.empty_like(like) if want_dres else None), torch.empty_like(like)
    ns = lib().cdll.ofa_join_bwd_slots(rows, cols, dtype_code(like))
    ws = torch.empty(5 * ns * cols, dtype=torch.float32, device=like.device)
    q = fold if fold is not None else FoldQueue()
    for i, o in enumerate(grads):
        if o is not None:
            q.add(ws, i * ns * cols, o, cols, cols, ns)
    want_xsum = len(grads) > 4 and grads[4] is not None
    lib().call("ofa_join_bwd", ptr(dy.contiguous() if dy is not None else None), ptr(dz.contiguous() if dz is not None else None),
               ptr(x), ptr(y), ptr(ga), ptr(gb), ptr(stats), ptr(keep), ptr(dres), ptr(dx), ptr(ws), rows, cols, float(p), seed, offset,
               ptr(offset_base), int(want_xsum), dtype_code(like), stream())
    if fold is None:
        q.flush()
    else:
        fold.flush_if_large()
    return dres, dx


# ------------------------------------------------------------------ generation steps (csrc/beam_search.hip, sample.hip, trie_beam.hip)
class _GenPolicy(ctypes.Structure):     # ofa_gen_policy
    _fields_ = [("temperature", ctypes.c_float), ("cstart", ctypes.c_int32), ("cend", ctypes.c_int32), ("step", ctypes.c_int32),
                ("min_len", ctypes.c_int32), ("max_len", ctypes.c_int32), ("pad", ctypes.c_int32), ("unk", ctypes.c_int32),
                ("eos", ctypes.c_int32), ("unk_penalty", ctypes.c_float), ("ngram", ctypes.c_int32), ("tokens", ctypes.c_void_p),
                ("tok_ld", ctypes.c_int64), ("done", ctypes.c_void_p)]


class _GenState(ctypes.Structure):      # ofa_gen_state
    _fields_ = [("tokens", ctypes.c_void_p), ("tok_ld", ctypes.c_int64), ("tok_cap", ctypes.c_int32), ("scores", ctypes.c_void_p),
                ("score_ld", ctypes.c_int64), ("ignore", ctypes.c_void_p), ("done", ctypes.c_void_p), ("nfin", ctypes.c_void_p),
                ("reorder", ctypes.c_void_p), ("fin_tok", ctypes.c_void_p), ("fin_pos", ctypes.c_void_p), ("fin_ld", ctypes.c_int64),
                ("fin_score", ctypes.c_void_p), ("fin_len", ctypes.c_void_p), ("fin_cnt", ctypes.c_void_p)]


def _gen_policy(step, tokens=None, done=None, temperature=1.0, constraint_range=None, min_len=1, max_len=256, pad=1, unk=3, eos=2,
                unk_penalty=0.0, ngram=0):
    """The row passes' ofa_gen_policy -> its address (the entry point copies it before it returns).  tokens: int64
    [rows, >= step + 1] history (n-gram bans); done: int32 [bsz] or None."""
    cs, ce = (-1, -1) if constraint_range is None else (int(constraint_range[0]), int(constraint_range[1]))
    p = _GenPolicy(float(temperature), cs, ce, int(step), int(min_len), int(max_len), int(pad), int(unk), int(eos), float(unk_penalty),
                   int(ngram), ptr(tokens), tokens.stride(0) if tokens is not None else 0, ptr(done))
    return ctypes.byref(p)


def _gen_state(st):
    """The sentence passes' ofa_gen_state from the state dict `st` (generator.SequenceGenerator._buffers, plus "tokens": the
    decoder's token history) -> (its address, bsz)."""
    tokens, scores, fin_tok = st["tokens"], st["scores"], st["fin_tok"]
    s = _GenState(ptr(tokens), tokens.stride(0), tokens.shape[1], ptr(scores), scores.stride(0), ptr(st["ignore"]), ptr(st["done"]),
                  ptr(st["nfin"]), ptr(st["reorder"]), ptr(fin_tok), ptr(st["fin_pos"]), fin_tok.stride(1), ptr(st["fin_score"]),
                  ptr(st["fin_len"]), ptr(st["fin_cnt"]))
    return ctypes.byref(s), st["done"].numel()


def beam_ws_bytes(rows, V, K):
    return int(lib().cdll.ofa_beam_ws_bytes(int(rows), int(V), int(K)))


def beam_topk(logits2d, K, step, ws, **policy):
    """Row pass of one beam-search step: logits2d [rows, V] (row stride ld, last dim contiguous) -> each row's normaliser parts and
    best 2K candidates in `ws` (beam_ws_bytes).  policy: _gen_policy's keywords."""
    rows, V = logits2d.shape
    if logits2d.stride(1) != 1:
        raise OfaError("beam_topk: the logits' last dimension must be contiguous")
    lib().call("ofa_beam_topk", ptr(logits2d), logits2d.stride(0), rows, V, int(K), _gen_policy(step, **policy), ptr(ws),
               dtype_code(logits2d), stream())


def beam_select(ws, st, K, V, step, max_len, eos=2, unk=3, unk_penalty=0.0, normalize=False, len_penalty=1.0):
    """Sentence pass of one beam-search step over the state dict `st` (_gen_state): finalises, selects the K active candidates,
    gathers the histories in place and writes the reorder index."""
    state, bsz = _gen_state(st)
    lib().call("ofa_beam_select", ptr(ws), state, bsz, int(K), int(V), int(step), int(max_len), int(eos), int(unk),
               float(unk_penalty), int(bool(normalize)), float(len_penalty), stream())


def beam_prefix_topk(logits2d, K, step, ws, plen, prefix=None, glogit=None, **policy):
    """beam_topk for a sample that carries prefix_tokens.  plen: int32 [bsz] prefix lengths (the n-gram bans skip rows with
    plen >= step + ngram - 1).  prefix int64 [bsz, > step] (a prefix step; None: a free step): no min_len mask, every row's scaled
    logit at prefix[sentence, step] goes to glogit fp32 [rows], and forced rows (prefix token != pad) get their candidates from
    beam_prefix_fill."""
    rows, V = logits2d.shape
    if logits2d.stride(1) != 1:
        raise OfaError("beam_prefix_topk: the logits' last dimension must be contiguous")
    if plen.dtype != torch.int32 or plen.numel() * int(K) != rows or not plen.is_contiguous():
        raise OfaError("beam_prefix_topk: plen must be a contiguous int32 [rows / K]")
    _check_prefix("beam_prefix_topk", prefix, glogit, rows, K)
    lib().call("ofa_beam_prefix_topk", ptr(logits2d), logits2d.stride(0), rows, V, int(K), _gen_policy(step, **policy), ptr(prefix),
               prefix.stride(0) if prefix is not None else 0, ptr(plen), ptr(glogit), ptr(ws), dtype_code(logits2d), stream())


def _check_prefix(who, prefix, glogit, rows, K):
    if prefix is None:
        return
    if prefix.dtype != torch.int64 or prefix.dim() != 2 or prefix.shape[0] * int(K) != rows or prefix.stride(1) != 1:
        raise OfaError(f"{who}: prefix must be int64 [rows / K, width] with a contiguous last dimension")
    if glogit is not None and (glogit.dtype != torch.float32 or glogit.numel() != rows or not glogit.is_contiguous()):
        raise OfaError(f"{who}: glogit must be a contiguous float32 [rows]")


def beam_prefix_fill(ws, rows, V, K, step, prefix, plen, glogit, **policy):
    """Between beam_prefix_topk and beam_prefix_select of a prefix step: the batch-wide fill value and the candidates of every
    forced row, written to `ws` as lprobs.  policy: the row pass's; tokens, done, pad, unk, unk_penalty and ngram are read."""
    _check_prefix("beam_prefix_fill", prefix, glogit, rows, K)
    lib().call("ofa_beam_prefix_fill", ptr(ws), int(rows), int(V), int(K), _gen_policy(step, **policy), ptr(prefix), prefix.stride(0),
               ptr(plen), ptr(glogit), stream())


def beam_prefix_select(ws, st, K, V, step, max_len, prefix, pad=1, eos=2, unk=3, unk_penalty=0.0, normalize=False, len_penalty=1.0):
    """beam_select of a prefix step: the candidate values of forced rows (prefix[sentence, step] != pad) are lprobs already."""
    state, bsz = _gen_state(st)
    _check_prefix("beam_prefix_select", prefix, None, bsz * int(K), K)
    lib().call("ofa_beam_prefix_select", ptr(ws), state, bsz, int(K), int(V), int(step), int(max_len), int(eos), int(unk),
               float(unk_penalty), int(bool(normalize)), float(len_penalty), ptr(prefix), prefix.stride(0), int(pad), stream())


# ------------------------------------------------------------------ closed-set scoring (csrc/closed_set_score.hip)
def closed_set_ws_bytes(bsz, E, N):
    return int(lib().cdll.ofa_closed_set_ws_bytes(int(bsz), int(E), int(N)))


def _closed_set_proj(h2d, weight, bias):
    if h2d.dim() != 2 or weight.dim() != 2 or h2d.stride(1) != 1 or weight.stride(1) != 1:
        raise OfaError("closed_set: features [rows, D] and projection rows [V, D] must have a contiguous last dimension")
    if weight.dtype != h2d.dtype or (bias is not None and bias.dtype != h2d.dtype):
        raise OfaError(f"closed_set: features ({h2d.dtype}), projection ({weight.dtype}) and bias must share one dtype")
    if weight.shape[1] != h2d.shape[1] or (bias is not None and (bias.numel() != weight.shape[0] or not bias.is_contiguous())):
        raise OfaError("closed_set: projection [V, D] / bias [V] do not match the features' width")


def closed_set_edge_logits(h2d, weight, bias, plan, bsz, chunk, T, c0, items, ws):
    """Stage 1 for one chunk of answers: h2d [bsz * chunk * T, D] holds the decoder features of answers c0 .. c0 + chunk - 1
    (row (b * chunk + c - c0) * T + t); `items` int32 [n, 3] is the slice of the plan's work items whose nodes are represented in
    the chunk; `plan`: the device arrays of a traverse.TraversePlan; ws: closed_set_ws_bytes(bsz, E, N) bytes."""
    _closed_set_proj(h2d, weight, bias)
    if h2d.shape[0] != bsz * chunk * T:
        raise OfaError(f"closed_set_edge_logits: {h2d.shape[0]} feature rows for bsz={bsz} x chunk={chunk} x T={T}")
    lib().call("ofa_closed_set_edge_logits", ptr(h2d), h2d.stride(0), dtype_code(h2d), ptr(weight), weight.stride(0), ptr(bias),
               h2d.shape[1], weight.shape[0], int(bsz), int(chunk), int(T), int(c0), ptr(items), items.shape[0],
               ptr(plan["edge_token"]), ptr(plan["rep_ans"]), ptr(plan["rep_pos"]), plan["N"], plan["E"], ptr(ws), stream())


def closed_set_reduce(plan, bsz, ws, scores):
    """Stages 2 and 3 over the edge logits in `ws`: scores fp32 [bsz, C] (contiguous)."""
    if scores.dtype != torch.float32 or not scores.is_contiguous() or scores.numel() != bsz * plan["C"]:
        raise OfaError("closed_set_reduce: scores must be a contiguous float32 [bsz, C]")
    lib().call("ofa_closed_set_reduce", int(bsz), plan["C"], plan["N"], plan["E"], plan["P"], ptr(plan["node_edge_off"]),
               ptr(plan["edge_node"]), ptr(plan["path_off"]), ptr(plan["path_edge"]), ptr(ws), ptr(scores), stream())


def closed_set_score(h2d, weight, bias, plan, bsz, ws=None):
    """All three stages for features that hold every answer: h2d [bsz * C * Tmax, D] -> scores fp32 [bsz, C]."""
    _closed_set_proj(h2d, weight, bias)
    C, T = plan["C"], plan["Tmax"]
    if h2d.shape[0] != bsz * C * T:
        raise OfaError(f"closed_set_score: {h2d.shape[0]} feature rows for bsz={bsz} x C={C} x Tmax={T}")
    if ws is None:
        ws = torch.empty((closed_set_ws_bytes(bsz, plan["E"], plan["N"]) + 3) // 4, dtype=torch.float32, device=h2d.device)
    scores = torch.empty(bsz, C, dtype=torch.float32, device=h2d.device)
    items = plan["items"]
    lib().call("ofa_closed_set_score", ptr(h2d), h2d.stride(0), dtype_code(h2d), ptr(weight), weight.stride(0), ptr(bias),
               h2d.shape[1], weight.shape[0], int(bsz), C, T, plan["N"], plan["E"], plan["P"], ptr(items), items.shape[0],
               ptr(plan["node_edge_off"]), ptr(plan["edge_token"]), ptr(plan["edge_node"]), ptr(plan["rep_ans"]),
               ptr(plan["rep_pos"]), ptr(plan["path_off"]), ptr(plan["path_edge"]), ptr(ws), ptr(scores), stream())
    return scores


# ------------------------------------------------------------------ sampling (csrc/sample.hip)
def sample_ws_bytes(rows, V, K):
    return int(lib().cdll.ofa_sample_ws_bytes(int(rows), int(V), int(K)))


def sample_draw(logits2d, K, step, ws, uniforms, topk=-1, topp=-1.0, **policy):
    """Row pass of one sampling step: logits2d [rows, V] and the policy as beam_topk takes them, uniforms fp32 [rows] (this step's
    number in [0, 1) per row) -> every row's drawn (lprob, token) in `ws` (sample_ws_bytes).  topp > 0 wins over topk > 0; neither:
    the whole vocabulary.  The draw is the inverse CDF of the kept weights in vocabulary order."""
    rows, V = logits2d.shape
    if logits2d.stride(1) != 1:
        raise OfaError("sample_draw: the logits' last dimension must be contiguous")
    if uniforms.dtype != torch.float32 or uniforms.numel() != rows or not uniforms.is_contiguous():
        raise OfaError("sample_draw: uniforms must be a contiguous float32 [rows]")
    lib().call("ofa_sample_draw", ptr(logits2d), logits2d.stride(0), rows, V, int(K), _gen_policy(step, **policy), int(topk),
               float(topp), ptr(uniforms), ptr(ws), dtype_code(logits2d), stream())


def sample_select(ws, st, K, step, max_len, eos=2, normalize=False, len_penalty=1.0):
    """Sentence pass of one sampling step over the state dict `st` (as beam_select): finalises the EOS draws, compacts the slots
    that go on to the front, gathers the histories in place and writes the reorder index."""
    state, bsz = _gen_state(st)
    lib().call("ofa_sample_select", ptr(ws), state, bsz, int(K), int(step), int(max_len), int(eos), int(bool(normalize)),
               float(len_penalty), stream())


# ------------------------------------------------------------------ diverse decoding (csrc/diverse_beam.hip)
def diverse_group_select(ws, st, K, V, step, max_len, groups, strength, eos=2, unk=3, unk_penalty=0.0, normalize=False,
                         len_penalty=1.0):
    """Sentence pass of one diverse-beam-search step, in place of beam_select after beam_topk: `groups` groups of K / groups beams
    (group g owns beams g, g + groups, ...), each penalised by strength (>= 0) times how often the groups before it took a token."""
    state, bsz = _gen_state(st)
    lib().call("ofa_diverse_group_select", ptr(ws), state, bsz, int(K), int(V), int(step), int(max_len), int(eos), int(unk),
               float(unk_penalty), int(bool(normalize)), float(len_penalty), int(groups), float(strength), stream())


def diverse_sibling_select(ws, st, K, V, step, max_len, rate, eos=2, unk=3, unk_penalty=0.0, normalize=False, len_penalty=1.0):
    """Sentence pass of one diverse-siblings step, in place of beam_select after beam_topk: after step 0 every beam's own top 2K
    continuations lose (rank + 1) * rate before the sentence's top 2K are taken."""
    state, bsz = _gen_state(st)
    lib().call("ofa_diverse_sibling_select", ptr(ws), state, bsz, int(K), int(V), int(step), int(max_len), int(eos), int(unk),
               float(unk_penalty), int(bool(normalize)), float(len_penalty), float(rate), stream())


# ------------------------------------------------------------------ trie-constrained beam search (csrc/trie_beam.hip)
def trie_beam_splits(max_degree, V):
    """Workgroups per row of trie_beam_topk for a plan (the grid's x extent)."""
    n = int(lib().cdll.ofa_trie_beam_splits(int(max_degree), int(V)))
    if n <= 0:
        raise OfaError(f"trie_beam_splits: max_degree={max_degree} V={V}")
    return n


def trie_beam_topk(h2d, weight, bias, plan, node, K, step, ws, **policy):
    """Row pass of one trie-constrained beam-search step, in place of beam_topk: h2d [rows, D] last-position features, weight
    [V, D] / bias the output projection, `plan` the device arrays of a traverse.TraversePlan, node int32 [rows] the trie node of
    every row (-1: dead); policy: _gen_policy's keywords but constraint_range (the trie is the constraint).  Writes `ws`
    (beam_ws_bytes(rows, V, K)) for beam_select of the same step."""
    _closed_set_proj(h2d, weight, bias)
    rows = h2d.shape[0]
    if node.dtype != torch.int32 or node.numel() != rows or not node.is_contiguous():
        raise OfaError("trie_beam_topk: node must be a contiguous int32 [rows]")
    lib().call("ofa_trie_beam_topk", ptr(h2d), h2d.stride(0), dtype_code(h2d), ptr(weight), weight.stride(0), ptr(bias),
               h2d.shape[1], weight.shape[0], rows, int(K), ptr(node), ptr(plan["node_edge_off"]), ptr(plan["edge_token"]),
               plan["N"], plan["E"], plan["max_degree"], _gen_policy(step, **policy), ptr(ws), stream())


def trie_beam_advance(plan, node, st, K, step):
    """After beam_select: every row's trie node follows its parent (st["reorder"]) through the token chosen at `step`; sentences
    with nothing left to finalise are marked done.  `st`: the state dict beam_select works on."""
    state, bsz = _gen_state(st)
    lib().call("ofa_trie_beam_advance", ptr(node), ptr(plan["node_edge_off"]), ptr(plan["edge_token"]), ptr(plan["edge_child"]),
               plan["N"], plan["E"], state, bsz, int(K), int(step), stream())


# ------------------------------------------------------------------ CTC loss on the encoder output (csrc/ctc.hip)
def ctc_limits():
    """(most classes, longest padded target row) the CTC kernels take."""
    c = lib().cdll
    return int(c.ofa_ctc_max_classes()), int(c.ofa_ctc_max_target())


def _ctc_rows2d(who, logits2d):
    if logits2d.dim() != 2 or logits2d.stride(1) != 1:
        raise OfaError(f"{who}: logits must be [rows, C] rows with a contiguous last dimension")
    C = logits2d.shape[1]
    if not 2 <= C <= ctc_limits()[0]:
        raise ValueError(f"{who}: C={C} classes; the CTC kernels take 2 .. {ctc_limits()[0]} (one float per class in LDS)")
    return logits2d.shape[0], C


def _ctc_seg(who, seg, row_stride, tmax):
    if seg.dtype != torch.int32 or seg.dim() != 2 or seg.shape[1] < 2 or seg.stride(1) != 1:
        raise OfaError(f"{who}: seg must be int32 [B, >= 2] = (row offset, length, ...) per sentence")
    if row_stride < 1 or not 0 <= tmax < 65536:
        raise ValueError(f"{who}: row_stride={row_stride}, tmax={tmax}")
    return seg.shape[0], (seg.stride(0) if seg.shape[0] > 1 else max(seg.stride(0), seg.shape[1]))


def ctc_rows(logits2d, want_argmax=False):
    """The row pass (ofa_ctc_rows): -> (row_lse fp64 [rows], row_argmax int32 [rows] or None; ties take the lowest class)."""
    rows, C = _ctc_rows2d("ctc_rows", logits2d)
    lse = torch.empty(rows, dtype=torch.float64, device=logits2d.device)
    am = torch.empty(rows, dtype=torch.int32, device=logits2d.device) if want_argmax else None
    lib().call("ofa_ctc_rows", ptr(logits2d), _ld(logits2d), rows, C, ptr(lse), ptr(am), dtype_code(logits2d), stream())
    return lse, am


def ctc_alpha_beta(logits2d, row_lse, seg, row_stride, tmax, target, ds, pad, eos, zero_infinity):
    """The two recursions (ofa_ctc_alpha_beta).  seg int32 [B, >= 2]: (row offset, length) of every sentence, rows off + t * row_stride,
    length <= tmax; target int64 [B, Lmax].  -> dict(alpha, beta fp64 [B, tmax, 2 Lmax + 1], meta, L: the labels as the gradient
    kernel reads them, nll_raw, nll64 fp64 [B], nll fp32 [B]: nll64 / nll have +inf replaced by 0 under zero_infinity)."""
    rows, C = _ctc_rows2d("ctc_alpha_beta", logits2d)
    B, seg_ld = _ctc_seg("ctc_alpha_beta", seg, row_stride, tmax)
    if target.dtype != torch.int64 or target.dim() != 2 or target.shape[0] != B or not target.is_contiguous() or target.shape[1] < 1:
        raise OfaError(f"ctc_alpha_beta: encoder_target must be a contiguous int64 [B={B}, Lmax >= 1], got {tuple(target.shape)}")
    Lmax = target.shape[1]
    if Lmax > ctc_limits()[1]:
        raise ValueError(f"ctc_alpha_beta: a target row of {Lmax} positions has {2 * Lmax + 1} states; the looped recursion takes "
                         f"{2 * ctc_limits()[1] + 1} (targets of up to {ctc_limits()[1]} positions)")
    dev = logits2d.device
    S = 2 * Lmax + 1
    st = dict(alpha=torch.empty(B, tmax, S, dtype=torch.float64, device=dev), beta=torch.empty(B, tmax, S, dtype=torch.float64, device=dev),
              meta=torch.empty(B, 3, Lmax, dtype=torch.int32, device=dev), L=torch.empty(B, dtype=torch.int32, device=dev),
              nll_raw=torch.empty(B, dtype=torch.float64, device=dev), nll=torch.empty(B, dtype=torch.float32, device=dev),
              nll64=torch.empty(B, dtype=torch.float64, device=dev), Lmax=Lmax)
    lib().call("ofa_ctc_alpha_beta", ptr(logits2d), _ld(logits2d), rows, C, ptr(row_lse), ptr(seg), seg_ld, int(row_stride), B, int(tmax),
               ptr(target), Lmax, int(ds), int(pad), int(eos), ptr(st["alpha"]), ptr(st["beta"]), ptr(st["meta"]), ptr(st["L"]),
               ptr(st["nll_raw"]), ptr(st["nll"]), ptr(st["nll64"]), int(bool(zero_infinity)), dtype_code(logits2d), stream())
    return st


def ctc_grad(logits2d, row_lse, seg, row_stride, tmax, st, seed, zero_infinity, out=None):
    """dlogits [rows, C] of the logits' dtype = seed[0] * d sum(nll) / d logits (ofa_ctc_grad); st: ctc_alpha_beta's result; seed: fp32
    device scalar or None (1).  Every row is written: exact zeros outside the sentences' lengths."""
    rows, C = _ctc_rows2d("ctc_grad", logits2d)
    B, seg_ld = _ctc_seg("ctc_grad", seg, row_stride, tmax)
    if out is None:
        out = torch.empty(rows, C, dtype=logits2d.dtype, device=logits2d.device)
    lib().call("ofa_ctc_grad", ptr(logits2d), _ld(logits2d), rows, C, ptr(row_lse), ptr(seg), seg_ld, int(row_stride), B, int(tmax),
               st["Lmax"], ptr(st["alpha"]), ptr(st["beta"]), ptr(st["meta"]), ptr(st["L"]), ptr(st["nll_raw"]), ptr(seed), ptr(out),
               out.stride(0) if rows > 1 else C, int(bool(zero_infinity)), dtype_code(logits2d), stream())
    return out


def ctc_greedy_decode(row_argmax, seg, row_stride, tmax):
    """-> (tokens int32 [B, tmax] with -1 behind each sentence's tokens, lengths int32 [B]) from the row pass's arg-max (ofa_ctc_greedy_decode)."""
    B, seg_ld = _ctc_seg("ctc_greedy_decode", seg, row_stride, tmax)
    if row_argmax.dtype != torch.int32 or not row_argmax.is_contiguous():
        raise OfaError("ctc_greedy_decode: row_argmax must be a contiguous int32 [rows]")
    out = torch.empty(B, tmax, dtype=torch.int32, device=row_argmax.device)
    n = torch.empty(B, dtype=torch.int32, device=row_argmax.device)
    lib().call("ofa_ctc_greedy_decode", ptr(row_argmax), row_argmax.numel(), ptr(seg), seg_ld, int(row_stride), B, int(tmax), ptr(out), ptr(n),
               stream())
    return out, n


# ------------------------------------------------------------------ text-to-speech: csrc/conv1d.hip, csrc/tacotron_loss.hip
def unfold1d(x, B, T, C, k):
    """x: batch-major channels-last rows [B*T, C] -> col [B*T, Kpad], taps ordered (k, c), padding (k-1)/2 inside every sample."""
    x = x.contiguous()
    if x.numel() != B * T * C:
        raise OfaError(f"unfold1d: {tuple(x.shape)} is not [B*T, C] = [{B}*{T}, {C}]")
    Kpad = (k * C + 7) // 8 * 8
    col = torch.empty(B * T, Kpad, dtype=x.dtype, device=x.device)
    lib().call("ofa_unfold1d", ptr(x), ptr(col), B, T, C, k, Kpad, dtype_code(x), stream())
    return col


def fold1d(dcol, B, T, C, k):
    """The adjoint of unfold1d: dcol [B*T, Kpad] -> dx [B*T, C], every element the fp32 sum of its <= k taps in tap order."""
    dcol = dcol.contiguous()
    if dcol.dim() != 2 or dcol.shape[0] != B * T or dcol.shape[1] < k * C or dcol.shape[1] % 8:
        raise OfaError(f"fold1d: {tuple(dcol.shape)} is not [B*T, Kpad] for B={B} T={T} C={C} k={k}")
    dx = torch.empty(B * T, C, dtype=dcol.dtype, device=dcol.device)
    lib().call("ofa_fold1d", ptr(dcol), ptr(dx), B, T, C, k, dcol.shape[1], dtype_code(dcol), stream())
    return dx


def tanh_dropout_fwd(x, p, seed, offset, offset_base=None):
    x = x.contiguous()
    y = torch.empty_like(x)
    lib().call("ofa_tanh_dropout_fwd", ptr(x), ptr(y), x.numel(), float(p), seed, offset, ptr(offset_base), dtype_code(x), stream())
    return y


def tanh_dropout_bwd(dy, y, p, seed, offset, offset_base=None):
    dy, y = dy.contiguous(), y.contiguous()
    if dy.shape != y.shape or dy.dtype != y.dtype:
        raise OfaError("tanh_dropout_bwd: dy and y differ in shape or dtype")
    dx = torch.empty_like(y)
    lib().call("ofa_tanh_dropout_bwd", ptr(dy), ptr(y), ptr(dx), y.numel(), float(p), seed, offset, ptr(offset_base), dtype_code(y),
               stream())
    return dx


TACOTRON_REDUCTIONS = {"mean": 0, "sum": 1}


def tacotron2_loss(feat_out, post, target, eos_out, lengths, bce_pos_weight, reduction, seed=None, grad=False, grads=None):
    """-> (out fp32 [4] = (loss, l1, mse, eos), (dfeat, dpost, deos) or None).  feat_out, post, target [B, T, F] and eos_out [B, T] (or
    [B, T, 1]) of one dtype, lengths int64 [B] on the device; seed: fp32 device scalar or None (1); grads: buffers to write into."""
    if reduction not in TACOTRON_REDUCTIONS:
        raise OfaError(f"tacotron2_loss: unknown reduction {reduction!r} (mean | sum)")
    if feat_out.dim() != 3 or post.shape != feat_out.shape or target.shape != feat_out.shape:
        raise OfaError(f"tacotron2_loss: feat_out {tuple(feat_out.shape)}, post {tuple(post.shape)} and target {tuple(target.shape)} "
                       "must be one [B, T, F]")
    B, T, F = feat_out.shape
    if eos_out.numel() != B * T:
        raise OfaError(f"tacotron2_loss: eos_out {tuple(eos_out.shape)} is not [B, T] = [{B}, {T}]")
    if post.dtype != feat_out.dtype or eos_out.dtype != feat_out.dtype:
        raise OfaError("tacotron2_loss: feat_out, post and eos_out must share one dtype")
    if lengths.dtype != torch.int64 or lengths.numel() != B:
        raise OfaError("tacotron2_loss: lengths must be int64 [B]")
    feat_out, post, target, eos_out, lengths = (t.contiguous() for t in (feat_out, post, target, eos_out, lengths))
    dev = feat_out.device
    nblocks = lib().cdll.ofa_tacotron2_loss_blocks(B * T, F)
    partial = torch.empty(max(nblocks, 1) * 3, dtype=torch.float64, device=dev)
    out = torch.empty(4, dtype=torch.float32, device=dev)
    d = None
    if grad:
        d = grads if grads is not None else (torch.empty_like(feat_out), torch.empty_like(post), torch.empty_like(eos_out))
    lib().call("ofa_tacotron2_loss", ptr(feat_out), ptr(post), ptr(target), ptr(eos_out), ptr(lengths), B, T, F, float(bce_pos_weight),
               TACOTRON_REDUCTIONS[reduction], ptr(seed), ptr(partial), ptr(out), ptr(d[0]) if grad else None,
               ptr(d[1]) if grad else None, ptr(d[2]) if grad else None, int(bool(grad)), dtype_code(feat_out), dtype_code(target),
               stream())
    return out, d


# ------------------------------------------------------------------ motion diffusion training: csrc/diffusion.hip
def _bool_mask(name, masks, B, T):
    if masks is None:
        return None
    if masks.dtype != torch.bool or tuple(masks.shape) != (B, T):
        raise OfaError(f"{name}: masks must be bool [B, T] = [{B}, {T}], got {masks.dtype} {tuple(masks.shape)}")
    return masks.contiguous()


def _levels(name, t, B):
    if t.dtype != torch.int64 or t.numel() != B:
        raise OfaError(f"{name}: the noise levels must be int64 [B] = [{B}], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def diffusion_q_sample(x0, noise, t, sqrt_acp, sqrt_1m_acp, width, dtype, known_w=None, masks=None):
    """-> the adaptor's input rows [B, T, width] of `dtype` (ofa_diffusion_q_sample).  x0, noise fp32 [B, T, Dd]; t int64 [B]; the two
    fp32 schedule tables; known_w fp32 [B, T] or None; masks bool [B, T] or None (masked frames: zeros)."""
    if x0.dim() != 3 or noise.shape != x0.shape or x0.dtype != torch.float32 or noise.dtype != torch.float32:
        raise OfaError(f"diffusion_q_sample: x0 {x0.dtype} {tuple(x0.shape)} and noise {noise.dtype} {tuple(noise.shape)} must be one fp32 "
                       "[B, T, Dd]")
    B, T, Dd = x0.shape
    if width < Dd:
        raise OfaError(f"diffusion_q_sample: data_dim {Dd} exceeds max_data_dim {width}")
    if sqrt_acp.dtype != torch.float32 or sqrt_1m_acp.dtype != torch.float32 or sqrt_acp.numel() != sqrt_1m_acp.numel():
        raise OfaError("diffusion_q_sample: the schedule tables must be fp32 of one length")
    if known_w is not None and (known_w.dtype != torch.float32 or tuple(known_w.shape) != (B, T)):
        raise OfaError(f"diffusion_q_sample: known_w must be fp32 [B, T] = [{B}, {T}], got {known_w.dtype} {tuple(known_w.shape)}")
    x0, noise, t, masks = x0.contiguous(), noise.contiguous(), _levels("diffusion_q_sample", t, B), _bool_mask("diffusion_q_sample", masks, B, T)
    known_w = known_w.contiguous() if known_w is not None else None
    out = torch.empty(B, T, int(width), dtype=dtype, device=x0.device)
    lib().call("ofa_diffusion_q_sample", ptr(x0), ptr(noise), ptr(t), ptr(known_w), ptr(masks), ptr(sqrt_acp.contiguous()),
               ptr(sqrt_1m_acp.contiguous()), sqrt_acp.numel(), B, T, Dd, int(width), ptr(out), dtype_code(out), stream())
    return out


def _film_args(name, h, rows, row_of):
    if h.dim() != 3 or rows.dim() != 2 or rows.shape[1] != 2 * h.shape[2] or rows.dtype != h.dtype:
        raise OfaError(f"{name}: h {h.dtype} {tuple(h.shape)} must be [B, T, D] and rows {rows.dtype} {tuple(rows.shape)} [R, 2D] of its dtype")
    B, T, D = h.shape
    if row_of is not None and (row_of.dtype != torch.int32 or tuple(row_of.shape) != (B, T)):
        raise OfaError(f"{name}: row_of must be int32 [B, T] = [{B}, {T}], got {row_of.dtype} {tuple(row_of.shape)}")
    return B, T, D, rows.shape[0]


def film_fwd(h, rows, row_of=None):
    """(rows[r, :D] + 1) * h + rows[r, D:] with r = row_of[b, t] (int32 [B, T]) or b (ofa_film_fwd)."""
    B, T, D, R = _film_args("film_fwd", h, rows, row_of)
    h, rows = h.contiguous(), rows.contiguous()
    row_of = row_of.contiguous() if row_of is not None else None
    out = torch.empty_like(h)
    lib().call("ofa_film_fwd", ptr(h), ptr(rows), ptr(row_of), B, T, D, R, ptr(out), dtype_code(h), stream())
    return out


def film_bwd(dout, h, rows, row_of=None):
    """-> (dh [B, T, D], drows [R, 2D]) of h's dtype (ofa_film_bwd).  With row_of, R = B + 1 and every entry is its sentence b or B."""
    B, T, D, R = _film_args("film_bwd", h, rows, row_of)
    if dout.shape != h.shape or dout.dtype != h.dtype:
        raise OfaError("film_bwd: dout and h differ in shape or dtype")
    dout, h, rows = dout.contiguous(), h.contiguous(), rows.contiguous()
    row_of = row_of.contiguous() if row_of is not None else None
    nch = (T + FILM_CHUNK - 1) // FILM_CHUNK
    partial = torch.empty(max(B * nch * (2 if row_of is not None else 1) * 2 * D, 1), dtype=torch.float32, device=h.device)
    dh, drows = torch.empty_like(h), torch.empty_like(rows)
    lib().call("ofa_film_bwd", ptr(dout), ptr(h), ptr(rows), ptr(row_of), B, T, D, R, ptr(dh), ptr(partial), ptr(drows), dtype_code(h),
               stream())
    return dh, drows


FILM_CHUNK = 16         # OFA_FILM_CHUNK of include/ofasys_amd.h: the frames a film_bwd workgroup sums (tests/test_diffusion_cpu.py compares the two)


def diffusion_loss(pred, target, t, w, scale, data_dim=None, masks=None, seed=None, grad=False, dpred=None):
    """-> (loss fp32 [1], dpred [B, T, W] of pred's dtype or None) (ofa_diffusion_loss).  pred [B, T, W] in the model dtype, read in
    place at columns < Dd; target fp32 [B, T, Dd]; t int64 [B]; w: the fp32 table sqrt(snr + 1), or None (the epsilon objective: weight
    1); masks bool [B, T] or None; seed: fp32 device scalar or None (1); dpred: a buffer to write into."""
    if pred.dim() != 3 or target.dim() != 3 or target.dtype != torch.float32 or pred.shape[:2] != target.shape[:2]:
        raise OfaError(f"diffusion_loss: pred {tuple(pred.shape)} must be [B, T, W] and target {target.dtype} {tuple(target.shape)} fp32 "
                       "[B, T, Dd]")
    B, T, W = pred.shape
    Dd = target.shape[2]
    if data_dim is not None and int(data_dim) != Dd:
        raise OfaError(f"diffusion_loss: data_dim {data_dim} is not the target's width {Dd}")
    if Dd > W:
        raise OfaError(f"diffusion_loss: the target is {Dd} wide, the prediction rows only {W}")
    if w is not None and w.dtype != torch.float32:
        raise OfaError("diffusion_loss: the weight table must be fp32")
    pred, target, masks = pred.contiguous(), target.contiguous(), _bool_mask("diffusion_loss", masks, B, T)
    t = _levels("diffusion_loss", t, B) if t is not None else None
    fpb = lib().cdll.ofa_diffusion_loss_frames(Dd)
    nblk = (T + fpb - 1) // fpb
    dev = pred.device
    partial = torch.empty(B * nblk, dtype=torch.float64, device=dev)
    counts = torch.empty(B, dtype=torch.float64, device=dev)
    out = torch.empty(1, dtype=torch.float32, device=dev)
    d = None
    if grad:
        d = dpred if dpred is not None else torch.empty_like(pred)
    lib().call("ofa_diffusion_loss", ptr(pred), ptr(target), ptr(t), ptr(masks), ptr(w.contiguous()) if w is not None else None,
               w.numel() if w is not None else 0, float(scale), ptr(seed), B, T, Dd, W, ptr(partial), ptr(counts), ptr(out), ptr(d),
               int(bool(grad)), dtype_code(pred), stream())
    return out, d


# ------------------------------------------------------------------ autoregressive speech generation (csrc/speech_step.hip)
class _SpeechStepArgs(ctypes.Structure):      # ofa_speech_step_args
    _fields_ = [("x", ctypes.c_void_p), ("ldx", ctypes.c_int64), ("feat_w", ctypes.c_void_p), ("feat_b", ctypes.c_void_p),
                ("eos_w", ctypes.c_void_p), ("eos_b", ctypes.c_void_p), ("pre_w", ctypes.c_void_p * 4), ("pre_b", ctypes.c_void_p * 4),
                ("proj_w", ctypes.c_void_p), ("proj_b", ctypes.c_void_p), ("feats", ctypes.c_void_p), ("eos_prob", ctypes.c_void_p),
                ("finished", ctypes.c_void_p), ("out_lens", ctypes.c_void_p), ("nfin", ctypes.c_void_p), ("pad_next", ctypes.c_void_p),
                ("embed", ctypes.c_void_p), ("offset_base", ctypes.c_void_p), ("threshold", ctypes.c_void_p), ("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64),
                ("offset_stride", ctypes.c_uint64), ("B", ctypes.c_int32), ("D", ctypes.c_int32), ("out_dim", ctypes.c_int32),
                ("P", ctypes.c_int32), ("E", ctypes.c_int32), ("layers", ctypes.c_int32), ("step", ctypes.c_int32),
                ("T_cap", ctypes.c_int32), ("p_drop", ctypes.c_float)]


def speech_step_rows():
    """Rows a workgroup of the step kernel owns (host only)."""
    return int(lib().cdll.ofa_speech_step_rows())


def speech_step_ok(D, out_dim, P, E, layers, dtype):
    """Does the fused step kernel serve this shape (host only)?  dtype: a torch dtype."""
    code = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}.get(dtype)
    return code is not None and int(lib().cdll.ofa_speech_step_route(int(D), int(out_dim), int(P), int(E), int(layers), code)) == 1


def speech_step(x, head, prenet, proj, state, step, p_drop, seed=0, offset=0, offset_stride=0, offset_base=None):
    """One launch of ofa_speech_step.  x [B, D] (rows may be strided); head = (feat_w, feat_b, eos_w, eos_b); prenet = [(w, b), ...];
    proj = (w, b); state: the generator's fixed-address buffers -- "feats" [B, T_cap, out_dim] and "embed" [B, E] of x's dtype,
    "eos_prob" fp32 [B, T_cap], "finished" / "out_lens" int32 [B], "nfin" int32 [1], "pad_next" bool / uint8 [B], "threshold" fp32 [1] (the finish test p > threshold)."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise OfaError("speech_step: x must be [B, D] rows")
    B, D = x.shape
    feat_w, feat_b, eos_w, eos_b = head
    feats, embed = state["feats"], state["embed"]
    tensors = [feat_w, feat_b, eos_w, eos_b, proj[0], proj[1], feats, embed] + [t for wb in prenet for t in wb]
    if any(t.dtype != x.dtype or not t.is_contiguous() for t in tensors):
        raise OfaError("speech_step: the weights, feats and embed must be contiguous tensors of x's dtype")
    out_dim, P, E = feat_w.shape[0], proj[0].shape[1], proj[0].shape[0]
    if (feat_w.shape[1] != D or eos_w.numel() != D or eos_b.numel() != 1 or feats.shape[0] != B or feats.shape[2] != out_dim
            or tuple(embed.shape) != (B, E) or tuple(state["eos_prob"].shape) != (B, feats.shape[1])
            or state["eos_prob"].dtype != torch.float32 or len(prenet) > 4
            or any(tuple(w.shape) != (P, out_dim if i == 0 else P) or b.numel() != P for i, (w, b) in enumerate(prenet))):
        raise OfaError("speech_step: shape mismatch between x, the weights and the state buffers")
    for name in ("finished", "out_lens", "nfin"):
        if state[name].dtype != torch.int32 or state[name].numel() != (1 if name == "nfin" else B):
            raise OfaError(f"speech_step: state['{name}'] must be int32 [{'1' if name == 'nfin' else 'B'}]")
    if state["threshold"].dtype != torch.float32 or state["threshold"].numel() != 1:
        raise OfaError("speech_step: state['threshold'] must be fp32 [1]")
    pad = state["pad_next"]
    if pad.numel() != B or pad.element_size() != 1 or not pad.is_contiguous():
        raise OfaError("speech_step: state['pad_next'] must be a contiguous bool / uint8 [B]")
    a = _SpeechStepArgs(x=ptr(x), ldx=x.stride(0), feat_w=ptr(feat_w), feat_b=ptr(feat_b), eos_w=ptr(eos_w), eos_b=ptr(eos_b),
                        proj_w=ptr(proj[0]), proj_b=ptr(proj[1]), feats=ptr(feats), eos_prob=ptr(state["eos_prob"]),
                        finished=ptr(state["finished"]), out_lens=ptr(state["out_lens"]), nfin=ptr(state["nfin"]), pad_next=ptr(pad),
                        embed=ptr(embed), offset_base=ptr(offset_base), threshold=ptr(state["threshold"]), seed=int(seed), offset=int(offset),
                        offset_stride=int(offset_stride), B=B, D=D, out_dim=out_dim, P=P, E=E, layers=len(prenet), step=int(step),
                        T_cap=feats.shape[1], p_drop=float(p_drop))
    for i, (w, b) in enumerate(prenet):
        a.pre_w[i], a.pre_b[i] = ptr(w), ptr(b)
    lib().call("ofa_speech_step", ctypes.addressof(a), dtype_code(x), stream())
