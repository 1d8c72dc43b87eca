"""torch.autograd.Function wrappers over the HIP kernels (ofasys_amd/kernels.py).

These are the building blocks the mirrored modules (ofasys_amd/module, adaptor, model) call.  Internally every
activation is a dense [rows, C] matrix in batch-major order ([B,T,C] storage); fairseq's [T,B,C] tensors at the module
boundary are transposed *views* of that storage, so no layout copies happen between ops.
"""

import weakref

import torch

from . import kernels as K
from .lib import OfaError


# ---------------------------------------------------------------------------------------------- layout helpers
def rows_view(x):
    """(x2d, restore): x2d is a contiguous [rows, C] view (or copy) of x; restore(y2d) gives y2d the shape/layout of x."""
    C = x.shape[-1]
    if x.is_contiguous():
        lead = x.shape[:-1]
        return x.view(-1, C), lambda y: y.view(*lead, y.shape[-1])
    if x.dim() == 3:
        xt = x.transpose(0, 1)
        if xt.is_contiguous():          # a [T,B,C] view of [B,T,C] storage
            b, t = xt.shape[0], xt.shape[1]
            return xt.view(-1, C), lambda y: y.view(b, t, y.shape[-1]).transpose(0, 1)
    xc = x.contiguous()
    lead = xc.shape[:-1]
    return xc.view(-1, C), lambda y: y.view(*lead, y.shape[-1])


def like_layout(x, ref):
    """x in the memory order of `ref` (same shape): rows_view() flattens each operand in ITS OWN storage order, so an element-wise
    row kernel over two operands needs both in one order -- a [T,B,C] tensor against a [T,B,C] view of [B,T,C] storage would
    otherwise pair row t*B+b with row b*T+t."""
    if x.dim() != 3 or x.shape != ref.shape:
        return x
    ref_bm = ref.transpose(0, 1).is_contiguous() and not ref.is_contiguous()
    x_bm = x.transpose(0, 1).is_contiguous() and not x.is_contiguous()
    if ref_bm == x_bm and (x_bm or x.is_contiguous() == ref.is_contiguous()):
        return x
    if ref_bm:
        return x.transpose(0, 1).contiguous().transpose(0, 1)
    return x.contiguous()


def batch_major(x):
    """[T,B,C] (any strides) -> contiguous [B,T,C] (a view when x is already a transposed batch-major buffer)."""
    xt = x.transpose(0, 1)
    return xt if xt.is_contiguous() else xt.contiguous()


class _Rng:
    """Philox (seed, offset) bookkeeping for dropout.  The stream position is `base` (a device int64, one per device) +
    `offset` (host, relative): kernels add the two on the device, so a captured (hipGraph) train step -- whose host
    arguments are frozen at capture time -- still draws fresh masks on every replay once the step ends with
    `advance()` (a captured device-side `base += offset`)."""
    seed = 0x5EED0FA
    offset = 0
    base = {}

    @classmethod
    def manual_seed(cls, seed):
        cls.seed, cls.offset = int(seed) & (2 ** 63 - 1), 0
        for b in cls.base.values():
            b.zero_()

    @classmethod
    def reserve(cls, n, device):
        o = cls.offset
        cls.offset += (n + 3) // 4 + 1
        b = cls.base.get(device)
        if b is None:
            b = cls.base[device] = torch.zeros(1, dtype=torch.int64, device=device)
        return cls.seed, o, b

    @classmethod
    def advance(cls):
        """Fold the relative offset consumed so far into the device-side base (call at the end of a train step)."""
        if cls.offset:
            for b in cls.base.values():
                b.add_(cls.offset)
            cls.offset = 0


    @classmethod
    def defer(cls):
        """advance() handed to a kernel that runs anyway: -> (base, offset) for the caller to add on the device (the relative offset is
        folded here), or None when there is nothing to add or more than one device's base (then advance() has run)."""
        if cls.offset and len(cls.base) == 1:
            (b,) = cls.base.values()
            o, cls.offset = cls.offset, 0
            return b, o
        cls.advance()
        return None


manual_seed = _Rng.manual_seed
rng_advance = _Rng.advance
rng_defer = _Rng.defer


# ---------------------------------------------------------------------------------------------- gradient sinks
# The train step (ofasys_amd/trainer.py) keeps every parameter gradient in one flat arena.  When a parameter carries
# `_ofa_grad` (its arena view), backward kernels ACCUMULATE straight into it (GEMM epilogue / reduce kernels with the
# accumulate flag) and return None to autograd: no temporary gradient tensor, no separate `grad += new` pass.
# `_ofa_grad_ready` (optional) tells the data-parallel reducer that one contribution has landed.
def _sink(param):
    return getattr(param, "_ofa_grad", None) if param is not None else None


def _sink_done(param):
    cb = getattr(param, "_ofa_grad_ready", None)
    if cb is not None:
        cb()


# First-touch gradient writes.  The train step does not clear the gradient arena.  Instead every launch that adds a result to a
# gradient asks `grad_mode` -- the ONE place that decides, at the moment the launch is issued (kernels._accum: the GEMM epilogues, the
# grouped launch's items, the fold jobs at their flush, the column sums and reduces) -- whether it stores or adds:
#   * the first FULL writer of a range of the arena in a step (a launch that writes every element of its view) stores;
#   * every later contribution adds: a second writer of a tied or shared parameter, a second micro-batch, a second chunk;
#   * a PARTIAL writer (embedding rows, a strided view) always adds; what nobody has written under it is cleared first;
#   * what nobody wrote at all by the end of backward is cleared then (`grad_end`): the unused-parameter rule.
# The touched set is a sorted list of disjoint element ranges of the arena, cleared per step (`grad_begin`).  The ranges a step had to
# clear on demand are handed back by `grad_end`; the next step of the same batch structure clears them up front in ONE launch.
# Values: storing round(x) and adding round(x) onto +0 give the same number (-0.0 stored where 0 + -0.0 gave +0.0 is the one difference in
# bits), so a step computes what it computed after an arena-wide zero fill.
class _Touched:
    arena = None         # the gradient arena of the running step (None: no step is running -- every sink adds)
    spans = []           # sorted, disjoint [lo, hi) element ranges written (or cleared) so far in this step
    demand = []          # ranges cleared on demand in this step, in order
    unused = []          # ranges nobody wrote (grad_end)


def _zero_ranges(arena, ranges, also=()):
    """Clear the element ranges of the arena (and the whole of every contiguous tensor in `also`) in one batched launch."""
    es = arena.element_size()
    K.zero_batched([(K.dptr(arena) + lo * es, (hi - lo) * es) for lo, hi in ranges] +
                   [(K.dptr(t), t.numel() * t.element_size()) for t in also])


def _span_gaps(lo, hi):
    """The parts of [lo, hi) outside the touched set."""
    import bisect
    spans, gaps = _Touched.spans, []
    i = bisect.bisect_right(spans, (lo, float("inf"))) - 1
    if i >= 0 and spans[i][1] > lo:
        lo = spans[i][1]
    i += 1
    while lo < hi:
        if i < len(spans) and spans[i][0] < hi:
            if spans[i][0] > lo:
                gaps.append((lo, spans[i][0]))
            lo = max(lo, spans[i][1])
            i += 1
        else:
            gaps.append((lo, hi))
            break
    return gaps


def _span_mark(lo, hi):
    import bisect
    spans = _Touched.spans
    i = bisect.bisect_left(spans, (lo, lo))
    if i > 0 and spans[i - 1][1] >= lo:
        i -= 1
    j = i
    while j < len(spans) and spans[j][0] <= hi:
        lo, hi = min(lo, spans[j][0]), max(hi, spans[j][1])
        j += 1
    spans[i:j] = [(lo, hi)]


def grad_begin(arena, prezero=(), also=()):
    """Start of a train step over the gradient arena `arena` (1-D): nothing is touched; `prezero` -- the ranges the previous step of this
    batch structure cleared on demand -- are cleared now, in one launch, before the first backward kernel.  also: small contiguous
    tensors the step wants cleared at its start (its statistics, the sum of squares), which ride in the same launch."""
    _Touched.arena, _Touched.spans, _Touched.demand, _Touched.unused = arena, [], [], []
    prezero = [(max(0, lo), min(arena.numel(), hi)) for lo, hi in prezero if lo < hi]
    if prezero or also:
        _zero_ranges(arena, prezero, also)
        for lo, hi in prezero:
            _span_mark(lo, hi)


def _dense(t):
    """Does the view cover every element of its memory range exactly once (contiguous in some order of its dimensions)?"""
    want = 1
    for n, st in sorted(((n, st) for n, st in zip(t.shape, t.stride()) if n > 1), key=lambda p: p[1]):
        if st != want:
            return False
        want *= n
    return True


def grad_mode(out, full=True, peek=False, store=False):
    """Does the launch being issued ADD to `out` (True) or is it the first full writer of that gradient in this step and stores (False)?
    Anything that is not a view of the running step's arena adds, as it always did.  peek: the answer alone, nothing is marked or cleared.
    store: the launch overwrites `out` whatever is there (accumulate=False): its range is marked as written -- a full view as it is, the
    unwritten rest under a strided one cleared first -- so that grad_end does not take it for a gradient nobody wrote."""
    arena = _Touched.arena
    if arena is None or out.dtype != arena.dtype or out.device != arena.device:
        return True
    es = arena.element_size()
    off = out.data_ptr() - arena.data_ptr()
    if off < 0 or off >= arena.numel() * es or out.numel() == 0:
        return True
    lo = off // es
    reach = 1 + sum((n - 1) * st for n, st in zip(out.shape, out.stride()))
    hi = lo + reach
    gaps = _span_gaps(lo, hi)
    if store and not peek and full and _dense(out):
        _span_mark(lo, hi)
        return False
    if full and _dense(out) and gaps == [(lo, hi)]:
        if not peek:
            _span_mark(lo, hi)
        return False
    if peek:
        return True
    if gaps:                                         # a partial writer, or a range written in part: clear the rest, then add
        _zero_ranges(arena, gaps)
        _Touched.demand.extend(gaps)
        _span_mark(lo, hi)
    return True


def grad_end():
    """End of a step's backward (every queued fold and weight gradient launched): clears what nobody wrote and closes the step.
    -> (ranges cleared on demand, ranges nobody wrote)."""
    arena = _Touched.arena
    if arena is None:
        return [], []
    _Touched.unused = _span_gaps(0, arena.numel())
    if _Touched.unused:
        _zero_ranges(arena, _Touched.unused)
    _Touched.arena = None
    return list(_Touched.demand), list(_Touched.unused)


def grad_abort():
    """A step that did not reach grad_end (backward raised): every sink adds again."""
    _Touched.arena = None


K.grad_mode = grad_mode


# Deferred folds (kernels.FoldQueue): when enabled, arena-gradient producers leave their fp32 partial rows in place and the
# queue reduces them in a handful of batched launches at the end of the backward pass.  Only legal when nothing consumes
# the gradients earlier -- i.e. not together with bucket all-reduces launched from inside backward.
class _Fold:
    queue = None
    queued = False


def defer_reductions(flag):
    if flag and _Fold.queue is None:
        _Fold.queue = K.FoldQueue()
    elif not flag and _Fold.queue is not None:
        flush_folds()
        _Fold.queue = None


def drop_pending():
    """Forget queued weight gradients and folds without launching them: the start of a step, so that what a backward pass that
    raised left behind is not added to the next step's gradients."""
    _Wgrads.items, _Wgrads.fillers, _Wgrads.queued, _Fold.queued = [], [], False, False
    if _Fold.queue is not None:
        _Fold.queue.__init__()


def flush_folds():
    flush_wgrads()
    _Fold.queued = False
    if _Fold.queue is not None:
        _Fold.queue.flush()


def _fold():
    """The active FoldQueue (or None); makes sure a flush runs when the current backward pass ends."""
    q = _Fold.queue
    if q is not None and not _Fold.queued:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(flush_folds)
            _Fold.queued = True
        except RuntimeError:
            return None                             # not inside a backward pass: reduce immediately
    return q


def _edge_fold():
    """_fold() for the column sums of the adaptors' backward (type vectors, patch-embedding bias and class token), which used to finish
    their sums themselves: queued with the immediate final pass's summation order (K.colsum(same_bits=True)), the same gradient bits."""
    return None if K.edge_old(K.EDGE_COLSUM_FOLD) else _fold()


# Grouped weight gradients: the nn.Linear weight gradients of a Transformer layer (dW += dY^T X into the arena) are
# collected while the layer's backward runs and launched together at a layer boundary (wgrad_boundary) -- one launch of
# 256 x 256 tiles (kernels.gemm_group_tn).  The queue holds dY and X until then.
# A boundary launches the queue only once it holds about a chip's worth of tiles (FLUSH_TILES of the 256 workgroups one
# round takes): a base-size layer is 108 (encoder) / 126 (decoder) tiles, so ONE layer per launch has to be cut into two
# K-slices per product to occupy the chip -- fp32 slabs written by the kernel and read back by a fold launch (23-27 us per
# layer on cfg-2, as long as two thirds of the decoder's grouped GEMM itself) -- while TWO layers are 216 / 252 workgroups
# of one slice each, accumulated straight onto the arena gradients in the epilogue: no slab, no fold.
# Cost of the deferral: the queue keeps one extra layer's dY / X operands alive until the next boundary -- per
# encoder layer of cfg-2 rows x (2304 + 3 * 768 + 2 * 3072 + 768 ... ) = 13312 rows x 12288 columns x 2 B = 327 MB (cfg-5, OFA-large
# at micro-batch 4: 1800 rows x 16384 x 2 B = 59 MB) of a 288 GB device -- and the weights of that layer report to the
# data-parallel reducer (`_sink_done`) one layer later: a bucket's all-reduce starts at most one layer's backward (~0.3 ms of a
# cfg-2 step) later than with a flush per layer; only the LAST bucket's delay is exposed, and that bucket ends with the embedding
# gradients, which are final only at the very end of backward anyway.
# FILLERS (round 6).  A pair of encoder layers is 216 workgroups of ONE round of the 256 CUs: 40 CUs idle for 315 us, three times per
# cfg-2 step -- while the weight gradient of the stack-wide cross-attention k|v projection (CrossKVShared: [L * 2D, D] over the same
# 13312 encoder rows, 108 tiles) ran as a launch of its own, 209 us, flushed ALONE out of the queue by the first decoder-side product
# behind it (another contraction length).  A product queued as a filler is cut into chunks of <= FILLER_TILES tiles (row blocks of the
# weight) that wait on the side; every group that leaves room in its round takes chunks of its own contraction length along: 216 + 36
# = 252 workgroups, the round costs what it cost, and the 209 us launch is gone.  Only while gradients are not consumed inside backward
# (no overlapped bucket all-reduces: a filler's parameters report to the reducer when its LAST chunk has been launched, which would
# hold back every bucket behind theirs).
class _Wgrads:
    enabled = True       # (tests / A-B tools may clear it: every weight gradient is then its own product)
    items = []           # (dy, x2d, out, alpha, weights, filler record or None)
    fillers = []         # chunks waiting for room: (dy view, x2d, out view, alpha, (), record); record = [chunks left, weights]
    queued = False       # an end-of-backward flush is registered with the autograd engine
    FLUSH_TILES = 128    # a boundary flushes a queue of more tiles than this (0: every boundary, rounds 3-4)
    FILLER_TILES = 40    # tiles per filler chunk (a group of two base-size encoder layers leaves 256 - 216 = 40)
    use_fillers = True   # (A/B tools may clear it)


def _tiles_of(dy, x2d):
    return ((dy.shape[1] + 255) // 256) * ((x2d.shape[1] + 255) // 256)


def _queued_tiles():
    return sum(_tiles_of(it[0], it[1]) for it in _Wgrads.items)


def _wgrad(dy, x2d, gw, alpha, *weights, filler=False):
    """gw += alpha * dy^T x2d (gw: the arena gradient of `weights` -- one weight, or several packed row-wise), then tell the
    reducer.  filler: nobody needs this gradient before the end of backward and later groups of the same contraction length are
    expected -- it may ride along with them in chunks (see _Wgrads)."""
    if _Wgrads.enabled and K.gemm_group_ok(dy, x2d, gw) and _flush_at_end_of_backward():
        tn = (x2d.shape[1] + 255) // 256
        if (filler and _Wgrads.use_fillers and _Fold.queue is not None and gw.dim() == 2 and dy.shape[1] % 256 == 0
                and tn <= _Wgrads.FILLER_TILES and _tiles_of(dy, x2d) > _Wgrads.FILLER_TILES):
            rows = max(1, _Wgrads.FILLER_TILES // tn) * 256                      # weight rows per chunk
            record = [0, weights]
            for r0 in range(0, dy.shape[1], rows):
                r1 = min(r0 + rows, dy.shape[1])
                _Wgrads.fillers.append((dy[:, r0:r1], x2d, gw[r0:r1], float(alpha), (), record))
                record[0] += 1
            return
        if _Wgrads.items and _Wgrads.items[0][0].shape[0] != dy.shape[0]:
            flush_wgrads()       # one contraction length per launch: the workgroup -> XCD map is by count (csrc/gemm_core.h group_enter), a group
                                 # mixing 13312-row and 3072-row products leaves some XCDs two rounds of long tiles and others idle
        _Wgrads.items.append((dy, x2d, gw, float(alpha), weights, None))
        if len(_Wgrads.items) == K.GROUP_MAX:
            flush_wgrads()
        return
    K.gemm(dy, x2d, True, False, alpha=alpha, out=gw, accumulate=True, fold=_fold())
    for w in weights:
        _sink_done(w)


def _flush_at_end_of_backward():
    """Makes sure whatever is still queued when the running backward pass ends is launched; False outside a backward pass."""
    if not _Wgrads.queued:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_end_of_backward)
            _Wgrads.queued = True
        except RuntimeError:
            return False
    return True


def _end_of_backward():
    _Wgrads.queued = False
    flush_wgrads()
    while _Wgrads.fillers:                           # chunks no group had room for: groups of their own, by contraction length
        rows = _Wgrads.fillers[0][0].shape[0]
        take = [f for f in _Wgrads.fillers if f[0].shape[0] == rows][:K.GROUP_MAX]
        _Wgrads.fillers = [f for f in _Wgrads.fillers if all(f is not t for t in take)]
        _Wgrads.items = take
        flush_wgrads(fill=False)


def flush_wgrads(fill=True):
    items, _Wgrads.items = _Wgrads.items, []
    if not items:
        return
    if fill and _Wgrads.fillers:
        # room left in the group's round of 256 workgroups: filler chunks of the same contraction length ride along
        rows, tiles = items[0][0].shape[0], sum(_tiles_of(it[0], it[1]) for it in items)
        rest = []
        for f in _Wgrads.fillers:
            t = _tiles_of(f[0], f[1])
            if f[0].shape[0] == rows and tiles + t <= 256 and len(items) < K.GROUP_MAX:
                items.append(f)
                tiles += t
            else:
                rest.append(f)
        _Wgrads.fillers = rest
    if len(items) == 1:
        dy, x2d, gw, alpha = items[0][:4]
        K.gemm(dy, x2d, True, False, alpha=alpha, out=gw, accumulate=True, fold=_fold())
    else:
        fold = _fold()
        q = fold if fold is not None else K.FoldQueue()
        K.gemm_group_tn([it[:4] for it in items], q)
        if fold is None:
            q.flush()                                # gradients are consumed from inside backward (bucket all-reduces): reduce now
        else:
            q.flush_if_large()
    for it in items:
        for w in it[4]:
            _sink_done(w)
        if it[5] is not None:                        # a filler chunk: its parameters are complete with the LAST chunk
            it[5][0] -= 1
            if it[5][0] == 0:
                for w in it[5][1]:
                    _sink_done(w)


class _WgradBoundaryFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        # (more than one more layer would not fit the group either: GROUP_MAX products)
        if _queued_tiles() > _Wgrads.FLUSH_TILES or 2 * len(_Wgrads.items) > K.GROUP_MAX:
            flush_wgrads()
        return dy


def wgrad_boundary(x):
    """Identity on a layer's input; in backward (when the layer's last gradient has been produced) the layer's queued weight
    gradients are launched as one group."""
    if _Wgrads.enabled and torch.is_grad_enabled() and x.requires_grad:
        return _WgradBoundaryFn.apply(x)
    return x


# ---------------------------------------------------------------------------------------------- LayerNorm
class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2d, weight, bias, eps, fuse_gelu):
        y, mean, rstd = K.layernorm_fwd(x2d, weight, bias, eps, fuse_gelu)
        ctx.save_for_backward(x2d, weight, mean, rstd)
        ctx.fuse_gelu = fuse_gelu
        ctx.bias_ref = bias
        return y

    @staticmethod
    def backward(ctx, dy):
        x2d, weight, mean, rstd = ctx.saved_tensors
        bias = ctx.bias_ref
        gw, gb = _sink(weight), _sink(bias)
        if gw is not None and gb is not None:
            dx = K.layernorm_bwd(dy, x2d, weight, mean, rstd, ctx.fuse_gelu, dgamma=gw, dbeta=gb, fold=_fold())[0]
            _sink_done(weight)
            _sink_done(bias)
            return dx, None, None, None, None
        dx, dg, db, _ = K.layernorm_bwd(dy, x2d, weight, mean, rstd, ctx.fuse_gelu)
        return dx, dg, db, None, None


class LayerNormForkFn(torch.autograd.Function):
    """(x, LayerNorm(x)): the pre-LN fork `residual = x; x = LN(x)` (transformer_layer.py:159-161, 186-188) as one node, so
    the gradient coming back through the residual branch is added inside the LayerNorm backward kernel instead of by a
    separate elementwise add."""

    @staticmethod
    def forward(ctx, x2d, weight, bias, eps):
        y, mean, rstd = K.layernorm_fwd(x2d, weight, bias, eps, False)
        ctx.save_for_backward(x2d, weight, mean, rstd)
        ctx.bias_ref = bias
        return x2d.view_as(x2d), y

    @staticmethod
    def backward(ctx, dres, dy):
        x2d, weight, mean, rstd = ctx.saved_tensors
        bias = ctx.bias_ref
        if dy is None:
            return dres, None, None, None
        gw, gb = _sink(weight), _sink(bias)
        if gw is not None and gb is not None:
            dx = K.layernorm_bwd(dy, x2d, weight, mean, rstd, False, dgamma=gw, dbeta=gb, fold=_fold(), dres=dres)[0]
            _sink_done(weight)
            _sink_done(bias)
            return dx, None, None, None
        dx, dg, db, _ = K.layernorm_bwd(dy, x2d, weight, mean, rstd, False, dres=dres)
        return dx, dg, db, None


def layer_norm_fork(x, weight, bias, eps=1e-5):
    """Returns (x, LayerNorm(x)) -- use the first as the residual."""
    x2d, restore = rows_view(x)
    r, y = LayerNormForkFn.apply(x2d, weight, bias, eps)
    return restore(r), restore(y)


class ResidualJoinFn(torch.autograd.Function):
    """(y, z) = (residual + dropout_p(LN_a(x)), LN_b(y)) in one pass each way (csrc/join.hip); LN_a / LN_b optional."""

    @staticmethod
    def forward(ctx, x2d, r2d, wa, ba, wb, bb, p, eps, x_bias=None):
        seed, off, base = (0, 0, None)
        if p > 0:
            seed, off, base = _Rng.reserve(x2d.numel(), x2d.device)
        y, z, stats, keep = K.join_fwd(x2d, r2d, (wa, ba) if wa is not None else None, (wb, bb) if wb is not None else None, eps,
                                       p, seed, off, base)
        ctx.save_for_backward(x2d if wa is not None else None, y if wb is not None else None, wa, wb, stats, keep)
        ctx.refs = (ba, bb, x_bias)
        ctx.rng = (p, seed, off, base)
        ctx.has_res = r2d is not None
        ctx.set_materialize_grads(False)                    # an unused y (last layer of a stack) costs no zero fill
        if z is None:
            return y, None
        return y, z

    @staticmethod
    def backward(ctx, dy, dz):
        if dy is None and dz is None:
            return (None,) * 9
        x2d, y, wa, wb, stats, keep = ctx.saved_tensors
        ba, bb, x_bias = ctx.refs
        p, seed, off, base = ctx.rng
        if wb is None:
            dz = None
        elif dz is None:
            dz = torch.zeros_like(y)
        params = (wa, ba, wb, bb)
        sinks = [(_sink(t) if t is not None else None) for t in params]
        use_sinks = all((t is None) or (s_ is not None) for t, s_ in zip(params, sinks))
        xb_sink = _sink(x_bias) if (x_bias is not None and use_sinks) else None      # bias gradient of x's Linear, fused
        if use_sinks:
            grads, fold = tuple(sinks) + (xb_sink,), _fold()
        else:
            grads = tuple((torch.zeros_like(t) if t is not None else None) for t in params)
            fold = None
        dres, dx = K.join_bwd(dy, dz, x2d, y, wa, wb, stats, p, seed, off, base, grads, fold, want_dres=ctx.has_res, keep=keep)
        if xb_sink is not None:
            _sink_done(x_bias)
        elif x_bias is not None:
            raise OfaError("residual_join: x_bias needs gradient sinks (the Linear skipped its own bias gradient)")
        if use_sinks:
            for t in params:
                if t is not None:
                    _sink_done(t)
            return dx, dres, None, None, None, None, None, None, None
        return dx, dres, grads[0], grads[1], grads[2], grads[3], None, None, None


def join_takes_bias_grad(*params):
    """True when a residual join may own the bias gradient of the Linear that feeds it: training with gradient sinks on
    every parameter involved (otherwise the Linear keeps its own column-sum pass)."""
    return torch.is_grad_enabled() and all(p is not None and p.requires_grad and _sink(p) is not None for p in params)


def residual_join(x, residual, ln_a, p, training, ln_b, eps=1e-5, x_bias=None):
    """Returns (y, z): y = residual + dropout(LN_a(x)) (LN_a: module or None), z = LN_b(y) (module or None -> z is None).
    x_bias: bias Parameter of the Linear that produced x when that Linear was called with skip_bias_grad=True -- its
    gradient (column sums of dx) then comes out of the join's backward kernel."""
    x2d, restore = rows_view(x)
    r2d = None
    if residual is not None:                                # (None: y = dropout(LN_a(x)), the adaptor post-hook)
        r2d, _ = rows_view(residual)
        if r2d.shape != x2d.shape:
            raise OfaError("residual_join: shape mismatch")
    wa, ba = (ln_a.weight, ln_a.bias) if ln_a is not None else (None, None)
    wb, bb = (ln_b.weight, ln_b.bias) if ln_b is not None else (None, None)
    y, z = ResidualJoinFn.apply(x2d, r2d, wa, ba, wb, bb, p if training else 0.0, eps, x_bias)
    return restore(y), (restore(z) if z is not None else None)


def layer_norm(x, weight, bias, eps=1e-5, fuse_gelu=False):
    """F.layer_norm over the last dim (module/layer_norm.py:27-32); fuse_gelu: LayerNorm(gelu(x))."""
    x2d, restore = rows_view(x)
    return restore(LayerNormFn.apply(x2d, weight, bias, eps, fuse_gelu))


# ---------------------------------------------------------------------------------------------- Linear
class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2d, weight, bias, alpha, skip_bias_grad=False):
        ctx.save_for_backward(x2d, weight)
        ctx.alpha = alpha
        ctx.has_bias = bias is not None and not skip_bias_grad      # (skipped: a downstream residual join produces it)
        ctx.bias_ref = bias
        N = weight.shape[0]
        out = None
        ctx.padded = False
        if N % 8 != 0:
            # ragged output width (vocabulary logits): pad the row stride to a multiple of 64 elements so the MFMA GEMMs
            # (LDS-DMA K tiles), the criterion and the gradient GEMMs stay vectorised; callers see the exact [rows, N] view.
            store = torch.empty(x2d.shape[0], (N + 63) // 64 * 64, dtype=x2d.dtype, device=x2d.device)
            out = store[:, :N]
            ctx.padded = True
        return K.gemm(x2d, weight, False, True, bias=bias, alpha=alpha, out=out)

    @staticmethod
    def backward(ctx, dy):
        x2d, weight = ctx.saved_tensors
        dy = dy if dy.stride(-1) == 1 else dy.contiguous()
        dx = dw = db = None
        N = weight.shape[0]
        # the criterion / probs kernels hand back a zero-padded gradient row (stride a multiple of 8)
        kpad = ctx.padded and dy.stride(0) >= (N + 7) // 8 * 8 and dy.stride(0) % 8 == 0   # zero tail up to the stride
        if ctx.needs_input_grad[0]:
            dx = K.gemm(dy, weight, False, False, alpha=ctx.alpha, a_kpad_zero=kpad)  # dX = dY W
        if ctx.needs_input_grad[1]:
            gw = _sink(weight)
            if gw is not None:                                                       # dW += dY^T X, in the arena
                _wgrad(dy, x2d, gw, ctx.alpha, weight)
            else:
                dw = K.gemm(dy, x2d, True, False, alpha=ctx.alpha)                   # dW = dY^T X
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = _sink(ctx.bias_ref)
            if gb is not None:
                K.colsum(dy, alpha=ctx.alpha, out=gb, accumulate=True, fold=_fold())
                _sink_done(ctx.bias_ref)
            else:
                db = K.colsum(dy, alpha=ctx.alpha, out_dtype=weight.dtype)
        return dx, dw, db, None, None


def linear(x, weight, bias=None, alpha=1.0, skip_bias_grad=False):
    """alpha * F.linear(x, weight, bias)."""
    x2d, restore = rows_view(x)
    return restore(LinearFn.apply(x2d, weight, bias, alpha, skip_bias_grad))


class LinearGeluLayerNormFn(torch.autograd.Function):
    """y = LayerNorm(gelu(x W^T + b)): fc1 -> GELU -> ffn_layernorm (transformer_layer.py:194-197).  Saves only the pre-GELU
    h; the backward LN kernel also produces the fc1 bias gradient (column sums of dh) from registers."""

    @staticmethod
    def forward(ctx, x2d, weight, bias, ln_w, ln_b, eps):
        h = K.gemm(x2d, weight, False, True, bias=bias)
        y, mean, rstd = K.layernorm_fwd(h, ln_w, ln_b, eps, True)
        ctx.save_for_backward(x2d, weight, h, ln_w, mean, rstd)
        ctx.refs = (bias, ln_b)
        return y

    @staticmethod
    def backward(ctx, dy):
        x2d, weight, h, ln_w, mean, rstd = ctx.saved_tensors
        bias, ln_b = ctx.refs
        gg, gb, gbias = _sink(ln_w), _sink(ln_b), _sink(bias)
        sunk = gg is not None and gb is not None and gbias is not None
        if sunk:
            dh = K.layernorm_bwd(dy, h, ln_w, mean, rstd, True, dgamma=gg, dbeta=gb, dbias=gbias, fold=_fold())[0]
            for p in (ln_w, ln_b, bias):
                _sink_done(p)
            dg = db = dbias = None
        else:
            dh, dg, db, dbias = K.layernorm_bwd(dy, h, ln_w, mean, rstd, True, want_dbias=True)
        dx = K.gemm(dh, weight, False, False) if ctx.needs_input_grad[0] else None
        gw = _sink(weight)
        dw = None
        if gw is not None:
            _wgrad(dh, x2d, gw, 1.0, weight)
        else:
            dw = K.gemm(dh, x2d, True, False)
        return dx, dw, dbias, dg, db, None


def linear_gelu_layer_norm(x, weight, bias, ln_w, ln_b, eps=1e-5):
    x2d, restore = rows_view(x)
    return restore(LinearGeluLayerNormFn.apply(x2d, weight, bias, ln_w, ln_b, eps))


# ---------------------------------------------------------------------------------------------- GELU / dropout / adds
class GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return K.gelu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return K.gelu_bwd(dy, x)


def gelu(x):
    x2d, restore = rows_view(x)
    return restore(GeluFn.apply(x2d))


class QuickGeluFn(torch.autograd.Function):
    """a = h * sigmoid(1.702 h) (module/vit.py QuickGELU); saves only h.  bias_param: the bias of the Linear that produced h, called with
    skip_bias_grad=True -- its gradient (the column sums of dh) leaves the backward kernel as partial rows for the fold when the
    parameter has an arena sink, and is a separate column sum handed to autograd when it has none."""

    @staticmethod
    def forward(ctx, h, bias_param):
        ctx.save_for_backward(h)
        ctx.bias_ref = bias_param
        return K.quick_gelu_fwd(h)

    @staticmethod
    def backward(ctx, dy):
        (h,) = ctx.saved_tensors
        bias = ctx.bias_ref
        if bias is None or not ctx.needs_input_grad[1]:
            return K.quick_gelu_bwd(dy, h), None
        gb = _sink(bias)
        if gb is not None and gb.is_contiguous():
            dh = K.quick_gelu_bwd(dy, h, dbias=gb, fold=_fold() or K.ImmediateFold())
            _sink_done(bias)
            return dh, None
        dh = K.quick_gelu_bwd(dy, h)
        return dh, K.colsum(dh, out_dtype=bias.dtype)


def quick_gelu(h, bias_param=None):
    """QuickGELU over the last dim's rows.  bias_param: see QuickGeluFn (the caller's Linear skipped its own bias gradient)."""
    h2d, restore = rows_view(h)
    return restore(QuickGeluFn.apply(h2d, bias_param))


class DropoutAddFn(torch.autograd.Function):
    """y = residual + dropout_p(x)  (residual may be None)."""

    @staticmethod
    def forward(ctx, x, residual, p):
        seed, off, base = _Rng.reserve(x.numel(), x.device)
        ctx.p, ctx.seed, ctx.off, ctx.base = p, seed, off, base
        ctx.has_res = residual is not None
        return K.dropout_add(x, residual, p, seed, off, base)

    @staticmethod
    def backward(ctx, dy):
        dx = K.dropout_bwd(dy, ctx.p, ctx.seed, ctx.off, ctx.base)
        return dx, (dy if ctx.has_res else None), None


class AddFn(torch.autograd.Function):
    """a + b + vec (row broadcast) with rows where rowmask is set forced to zero.  b may hold the rows of ONE sample (fewer rows than a:
    positions shared by the batch) -- it is then read with a period and its gradient is the sum over the batch."""

    @staticmethod
    def forward(ctx, a, b, vec, rowmask, vec_param=None, b_range=None):
        ctx.save_for_backward(rowmask)
        ctx.has = (b is not None, vec is not None)
        ctx.vdtype = vec.dtype if vec is not None else None
        ctx.b_shape = tuple(b.shape) if (b is not None and b.numel() != a.numel()) else None
        ctx.vec_param = vec_param                      # the parameter `vec` is a view of: its gradient goes straight to the arena
        # (table, r0): the batch-shared b is rows r0 .. of `table`, looked up by arange (ops.embedding(range_start=)) and handed in
        # detached -- its gradient, summed over the batch, is added to the table's arena gradient by ONE kernel here
        ctx.b_range = b_range
        return K.add_rowvec_mask(a, b, vec, rowmask)

    @staticmethod
    def backward(ctx, dy):
        (rowmask,) = ctx.saved_tensors
        g = K.add_rowvec_mask(dy, None, None, rowmask) if rowmask is not None else dy
        dvec = None
        if ctx.has[1]:
            gv = _sink(ctx.vec_param)
            if gv is not None and gv.is_contiguous():
                K.colsum(g, out=gv.view(-1), accumulate=True, fold=_edge_fold(), same_bits=True)
                _sink_done(ctx.vec_param)
            else:
                dvec = K.colsum(g, out_dtype=ctx.vdtype)
        db = None
        if ctx.b_range is not None:
            table, r0 = ctx.b_range
            K.embedding_range_bwd(g, _sink(table), r0, ctx.b_shape[0])
            _sink_done(table)
        elif ctx.has[0]:
            if ctx.b_shape is None:
                db = g
            else:
                nb = 1
                for d in ctx.b_shape:
                    nb *= d
                db = K.batch_sum(g, g.numel() // nb).view(ctx.b_shape)
        return g, db, dvec, None, None, None


def dropout_add(x, residual, p, training):
    """residual + dropout(x) (transformer_layer.py:181-182); plain add when not training / p == 0."""
    if residual is not None:
        x = like_layout(x, residual)
    x2d, restore = rows_view(x)
    r2d = None
    if residual is not None:
        r2d, _ = rows_view(residual)
        if r2d.shape != x2d.shape:
            raise OfaError("dropout_add: shape mismatch")
    if training and p > 0:
        return restore(DropoutAddFn.apply(x2d, r2d, p))
    if r2d is None:
        return x
    return restore(AddFn.apply(x2d, r2d, None, None))


def shared_rows(x):
    """[1, T, D] base of a [B, T, D] tensor whose B samples are one and the same storage (a stride-0 `expand`: position embeddings of
    arange- / grid-derived positions, which every built-in adaptor returns that way), else None."""
    if x is not None and x.dim() == 3 and x.shape[0] > 1 and x.stride(0) == 0:
        # the tensor the expand was taken of, when autograd still knows it: going through `x[:1]` instead would make backward zero-fill
        # a [B, T, D] gradient, copy one sample into it and sum it over the batch again
        base = x._base
        if (base is not None and base.dim() == 3 and base.shape[0] == 1 and tuple(base.shape[1:]) == tuple(x.shape[1:])
                and base.data_ptr() == x.data_ptr() and base.stride()[1:] == x.stride()[1:]):
            return base
        return x[:1]
    return None


def first_sample(x):
    """x[:1] of a [B, T, D] tensor -- through the base of a batch-shared tensor when it is one (see shared_rows)."""
    base = shared_rows(x)
    return base if base is not None else x[:1]


def _range_sink(b):
    """(table, r0) when the [1, T, D] tensor b is ops.embedding(range_start=r0)'s output -- rows r0 .. r0 + T - 1 of `table`, by the caller's
    promise -- and the table has a contiguous arena gradient the range kernel can add to; else None."""
    rng = getattr(b, "_ofa_range", None)
    if rng is None or not b.requires_grad or not b.is_contiguous():
        return None
    gw = _sink(rng[0])
    if gw is None or not gw.is_contiguous() or gw.dtype != b.dtype or not K.embedding_range_ok(b):
        return None
    return rng


def add_rowvec_mask(a, b=None, vec=None, rowmask=None, vec_param=None):
    """a [B, T, D] + b + vec: b is [B, T, D] or -- batch-shared -- [1, T, D] / a stride-0 expand of it (read once per sample, never
    materialised B times; its gradient comes back summed over the batch).  vec_param: the parameter `vec` is a flat view of (its
    gradient is then accumulated into the gradient arena by the op's own backward)."""
    if vec_param is not None and not (vec is not None and vec.requires_grad and torch.is_grad_enabled() and _sink(vec_param) is not None):
        vec_param = None                               # (no gradient arena: autograd carries the gradient as usual)
    if vec_param is not None:
        vec = vec.detach()                             # the gradient takes the direct route
    if b is not None:
        base = shared_rows(b)
        if base is not None and a.dim() == 3 and a.is_contiguous() and tuple(a.shape[1:]) == tuple(base.shape[1:]):
            b = base
        if b.shape[0] == 1 and a.dim() == 3 and a.shape[0] > 1 and a.is_contiguous() and tuple(a.shape[1:]) == tuple(b.shape[1:]):
            m = rowmask.reshape(-1) if rowmask is not None else None
            b_range = _range_sink(b) if (a.requires_grad and torch.is_grad_enabled()) else None
            if b_range is not None:
                b = b.detach()                         # the gradient takes the direct route
            return AddFn.apply(a.view(-1, a.shape[-1]), b.reshape(-1, b.shape[-1]), vec, m, vec_param, b_range).view(a.shape)
        b = like_layout(b, a)
    a2d, restore = rows_view(a)
    b2d = rows_view(b)[0] if b is not None else None
    m = rowmask.reshape(-1) if rowmask is not None else None
    return restore(AddFn.apply(a2d, b2d, vec, m, vec_param))


class DropPathFn(torch.autograd.Function):
    """x * scale[sample] on batch-major rows (module/droppath.py:40-60: scale = floor(keep + U[0,1)) / keep per sample)."""

    @staticmethod
    def forward(ctx, x2d, scale, group):
        ctx.save_for_backward(scale)
        ctx.group = group
        return K.scale_row_groups(x2d, scale, group)

    @staticmethod
    def backward(ctx, dy):
        (scale,) = ctx.saved_tensors
        return K.scale_row_groups(dy.contiguous(), scale, ctx.group), None, None


def _drop_path_uniform(B, device):
    """The U[0,1) draw per sample of module/droppath.py:52 (a seam: the parity tests replay the reference's recorded draws here)."""
    return torch.rand(B, dtype=torch.float32, device=device)


def drop_path(x, drop_prob, batch_axis=1, scale_by_keep=True):
    """Per-sample stochastic depth of a [T,B,C] (batch_axis=1) or [B,T,C] (batch_axis=0) activation."""
    keep = 1.0 - drop_prob
    B = x.shape[batch_axis]
    mask = (keep + _drop_path_uniform(B, x.device)).floor_()
    if keep > 0.0 and scale_by_keep:
        mask = mask / keep
    xb = batch_major(x) if batch_axis == 1 else x.contiguous()          # [B,T,C]: one sample = T consecutive rows
    T, C = xb.shape[1], xb.shape[2]
    y = DropPathFn.apply(xb.view(B * T, C), mask, T).view(B, T, C)
    return y.transpose(0, 1) if batch_axis == 1 else y


# ---------------------------------------------------------------------------------------------- embedding
def cached_index(owner, key, make):
    """Constant integer index tensors derived from a module's buffers and a shape (rel-pos bucket windows): built once per (owner,
    key, device) instead of by one slicing / gather launch per layer and step.  Nothing is inserted while a graph is being captured
    (the tensor would belong to that graph's pool and only hold data after its replay)."""
    cache = owner.__dict__.setdefault("_ofa_index_cache", {})
    hit = cache.get(key)
    if hit is not None:
        ref = next(owner.buffers(), None)
        ref = ref if ref is not None else next(owner.parameters(), None)
        if ref is None or hit.device == ref.device:
            return hit
    t = make()
    if not (t.is_cuda and torch.cuda.is_current_stream_capturing()):
        if len(cache) >= 64:
            cache.clear()
        cache[key] = t
    return t


def owner_token(owner):
    """A hashable identity of `owner` (a module) for process-wide caches.  NOT id(owner): ids are recycled after garbage collection,
    and a later model whose adaptor lands on a freed address (another bucket table, the same T) would be handed the stale plan
    (ADVICE r3).  The token object lives in the owner's __dict__ and in every cache key built from it, so its identity cannot be
    reused while an entry exists; a copy.deepcopy / pickled module gets a fresh one."""
    tok = owner.__dict__.get("_ofa_owner_token")
    if tok is None or tok.owner_id != id(owner):
        tok = owner.__dict__["_ofa_owner_token"] = _OwnerToken(id(owner))
        # entries keyed by the token go when the owner does (a process that builds many models -- tests, sweeps -- would otherwise keep
        # every dead model's plan tensors on the device: ADVICE r4).  The finalizer holds the token, not the owner.
        weakref.finalize(owner, _purge_owner_entries, tok)
    return tok


def _purge_owner_entries(tok):
    def mentions(key):
        return key is tok or (isinstance(key, tuple) and any(mentions(k) for k in key))
    for cache in _TOKEN_KEYED_CACHES:
        for key in [k for k in cache if mentions(k)]:
            del cache[key]


_TOKEN_KEYED_CACHES = []        # process-wide caches whose keys contain owner tokens (SegmentPlan._cache registers itself below)


class _OwnerToken:
    __slots__ = ("owner_id",)

    def __init__(self, owner_id):
        self.owner_id = owner_id

    def __deepcopy__(self, memo):
        return _OwnerToken(-1)                       # the copy's owner_token() replaces it on first use


class SegmentPlan:
    """The positions of an id tensor sorted by id (stable) and cut into one segment per distinct id: what ofa_segment_rowsum needs to
    scatter-add a narrow table's gradient without scanning the id list per table row.  Built on the device (sort + unique) with ONE
    host sync for the segment count -- once per lookup: the ids of a rel-pos bias (bucket[:T, :T]) are the same every step."""
    _cache = {}

    def __init__(self, ids):
        flat = ids.reshape(-1)
        assert flat.numel() < 2 ** 31
        sorted_ids, order = torch.sort(flat, stable=True)
        rows, counts = torch.unique_consecutive(sorted_ids, return_counts=True)
        self.nseg = int(rows.numel())                                    # (the sync)
        self.order = order.to(torch.int32)
        self.seg_row = rows.to(torch.int32)
        off = torch.zeros(self.nseg + 1, dtype=torch.int32, device=ids.device)
        off[1:] = torch.cumsum(counts, 0).to(torch.int32)
        self.seg_off = off
        self.min_row, self.max_row = (int(rows.min()), int(rows.max())) if self.nseg else (0, -1)

    @classmethod
    def get(cls, key, ids):
        """The cached plan of lookup `key`; None while a hipGraph is being captured and the plan does not exist yet (building it
        syncs), in which case the caller takes the scan kernel."""
        plan = cls._cache.get(key)
        if plan is None:
            if ids.is_cuda and torch.cuda.is_current_stream_capturing():
                return None
            if len(cls._cache) > 512:
                cls._cache.clear()
            plan = cls._cache[key] = cls(ids)
        return plan


_TOKEN_KEYED_CACHES.append(SegmentPlan._cache)


class EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, weight, padding_idx, plan_key=None, pad_mask_of=None, range_start=None):
        ctx.save_for_backward(ids)
        ctx.V, ctx.padding_idx = weight.shape[0], padding_idx
        ctx.weight_ref = weight
        ctx.plan_key = plan_key
        ctx.range_start = range_start
        ctx.with_mask = pad_mask_of is not None
        ctx.set_materialize_grads(False)               # (the mask output has no gradient: no zero fill of one per backward)
        if pad_mask_of is None:
            return K.embedding_fwd(weight, ids)
        out, mask = K.embedding_fwd(weight, ids, pad_mask_of)          # the ids' padding mask from the same pass
        ctx.mark_non_differentiable(mask)
        return out, mask

    @staticmethod
    def backward(ctx, dout, *_unused):
        if dout is None:
            return (None,) * 6
        return EmbeddingFn._backward(ctx, dout) + (None, None)

    @staticmethod
    def _backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        pad = -1 if ctx.padding_idx is None else ctx.padding_idx
        gw = _sink(ctx.weight_ref)
        D = dout.shape[-1]
        if (ctx.range_start is not None and ctx.padding_idx is None and K.embedding_range_ok(dout)
                and (gw is None or (gw.is_contiguous() and gw.dtype == dout.dtype))):
            # ids are range_start .. range_start + n - 1 by the caller's promise: row t of dout is the gradient of table row range_start + t
            out = gw if gw is not None else torch.zeros(ctx.V, D, dtype=dout.dtype, device=dout.device)
            K.embedding_range_bwd(dout.reshape(-1, D), out, ctx.range_start, ids.numel())
            if gw is not None:
                _sink_done(ctx.weight_ref)
                return None, None, None, None
            return None, out, None, None
        plan = None
        if ctx.plan_key is not None and D <= 64 and ctx.padding_idx is None:
            plan = SegmentPlan.get((ctx.plan_key, tuple(ids.shape), str(ids.device)), ids)
            if plan is not None and not (0 <= plan.min_row and plan.max_row < ctx.V):
                plan = None
        if plan is not None:                                            # narrow table, ids known in advance: one wave per distinct id
            d2 = dout.reshape(-1, D)
            d2 = d2 if d2.is_contiguous() else d2.contiguous()
            if gw is not None:
                K.segment_rowsum(d2, plan, gw, True)
                _sink_done(ctx.weight_ref)
                return None, None, None, None
            return None, K.segment_rowsum(d2, plan, torch.zeros(ctx.V, D, dtype=dout.dtype, device=dout.device), False), None, None
        if gw is not None:
            K.embedding_bwd(dout, ids, ctx.V, pad, dweight=gw)       # the kernel accumulates into dweight
            _sink_done(ctx.weight_ref)
            return None, None, None, None
        dw = K.embedding_bwd(dout, ids, ctx.V, pad)
        return None, dw, None, None


def embedding(ids, weight, padding_idx=None, plan_key=None, range_start=None):
    """F.embedding.  plan_key (hashable, optional): promises that every call with this key and shape looks up the SAME ids (a rel-pos
    bucket table slice) -- the gradient then uses a cached sort of the ids (SegmentPlan) instead of scanning them per table row.
    range_start (int, optional): promises that ids IS arange(range_start, range_start + ids.numel()) (positions; nothing checks it) --
    the gradient of table row range_start + t is then row t of the output's, added without a scatter, and a consumer that broadcasts the
    rows over a batch (add_rowvec_mask) sums its gradient over the batch in the same kernel."""
    if range_start is None:
        return EmbeddingFn.apply(ids, weight, padding_idx, plan_key)
    out = EmbeddingFn.apply(ids, weight, padding_idx, plan_key, None, int(range_start))
    if ids.dim() == 2 and ids.shape[0] == 1 and padding_idx is None:
        out._ofa_range = (weight, int(range_start))
    return out


def embedding_with_pad_mask(ids, weight, padding_idx, pad):
    """(F.embedding(ids), ids == pad) in one launch (adaptor/text.py:108-125)."""
    return EmbeddingFn.apply(ids, weight, padding_idx, None, int(pad))


# ---------------------------------------------------------------------------------------------- attention
def _c_attn_grad(delta, c_attn, B, heads, T):
    """d c_attn[h] = sum_{b,t} rowsum(dO*O)[b,h,t] / c[h]  (O = c * PV): one kernel, straight into the gradient arena when
    the parameter has a sink (returns None then)."""
    g = _sink(c_attn)
    if g is not None:
        K.c_attn_grad(delta, c_attn, B, heads, T, out=g, accumulate=True)
        _sink_done(c_attn)
        return None
    return K.c_attn_grad(delta, c_attn, B, heads, T)


def _split_seg(kpm):
    """The key-padding argument of the attention functions is either a mask tensor (padded batches) or a packing.Segments
    table (ragged batches, ofasys_amd/packing.py).  -> (mask tensor or None, Segments or None)"""
    if kpm is not None and not torch.is_tensor(kpm):
        return None, kpm
    return kpm, None


class PackRowsFn(torch.autograd.Function):
    """[rows_in, D] -> [rows_out, D] row gather with zero fill (index -1); backward = the same gather with the inverse index
    (packing.PackPlan.*_index / *_inverse)."""

    @staticmethod
    def forward(ctx, x2d, index, inverse):
        ctx.save_for_backward(inverse)
        return K.gather_rows(x2d, index)

    @staticmethod
    def backward(ctx, dout):
        (inverse,) = ctx.saved_tensors
        return K.gather_rows(dout.contiguous(), inverse), None, None


class PackPartsFn(torch.autograd.Function):
    """Packed rows of torch.cat(parts, dim=1) without the concatenation: one gather over the slots' own [B, n_k, D] outputs
    (K.gather_rows_parts); backward hands every part its contiguous [B, n_k, D] gradient (K.scatter_rows_part)."""

    @staticmethod
    def forward(ctx, index, inverse, *parts):
        ctx.save_for_backward(inverse)
        ctx.lens = [int(t.shape[1]) for t in parts]
        ctx.B = parts[0].shape[0]
        return K.gather_rows_parts([t.contiguous() for t in parts], index)

    @staticmethod
    def backward(ctx, dout):
        (inverse,) = ctx.saved_tensors
        d = dout.contiguous()
        T, grads, s = sum(ctx.lens), [], 0
        for i, n in enumerate(ctx.lens):
            grads.append(K.scatter_rows_part(d, inverse, ctx.B, n, T, s) if ctx.needs_input_grad[2 + i] else None)
            s += n
        return (None, None) + tuple(grads)


class LazyCat:
    """torch.cat(parts, dim=1) that has not happened yet: what the general adaptor hands the encoder / decoder stacks as `embed` when
    they asked for it (row packing: the packed rows are gathered from the parts directly).  `.materialize()` is the tensor."""

    def __init__(self, parts):
        self.parts = list(parts)
        B, _, D = self.parts[0].shape
        self.shape = torch.Size((B, sum(int(t.shape[1]) for t in self.parts), D))
        self.dtype, self.device = self.parts[0].dtype, self.parts[0].device

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def materialize(self):
        return torch.cat(tuple(self.parts), dim=1)


def materialize(x):
    return x.materialize() if isinstance(x, LazyCat) else x


def pack_rows(x, index, inverse):
    """x [B, T, D] (padded; a tensor or a LazyCat of the slots' outputs) -> [1, R, D] packed rows."""
    B, T, D = x.shape
    if isinstance(x, LazyCat):
        # (slots whose embeddings differ in dtype or batch -- an fp32 adaptor beside 16-bit text, which torch.cat would promote -- take
        #  the materialised path: the parts gather reads every part as ONE dtype)
        if len(x.parts) <= 8 and D % 8 == 0 and all(t.is_cuda and t.dtype == x.parts[0].dtype and t.shape[0] == B and t.dim() == 3
                                                    for t in x.parts):
            return PackPartsFn.apply(index, inverse, *x.parts).view(1, -1, D)
        x = x.materialize()
    return PackRowsFn.apply(x.reshape(B * T, D), index, inverse).view(1, -1, D)


def _dbias_dtype(bias, shared):
    """A shared bias' batch-summed gradient leaves the kernels in the bias' own dtype (the chunk fold casts): no separate cast launch."""
    return bias.dtype if (shared and bias is not None) else torch.float32


def _shared_dbias(dbias, bias, shared):
    """The batch-summed dS of a shared bias comes back as fp32 [heads, Tb, Sb]: in the bias' own dtype and shape for autograd."""
    if dbias is None or not shared:
        return dbias
    return dbias.to(bias.dtype).view(bias.shape)


class _AttnCs:
    """Partial-row buffers of one attention backward call (kernels.attn_bwd cs=): bufs = the dict handed to the kernels, bias_ws /
    c_ws = the fp32 buffers to register with the queue fq (None: that gradient takes the separate-pass route), ns = partial rows.
    As constructed: empty -- both gradients take the separate pass."""
    __slots__ = ("bufs", "bias_ws", "c_ws", "ns", "fq")

    def __init__(self):
        self.bufs, self.bias_ws, self.c_ws, self.ns, self.fq = {}, None, None, 0, None


def _attn_cs_begin(gb, c_ref, B, T, S, seg, heads, dev, order=None):
    """-> _AttnCs.  gb: the arena gradient of the call's packed bias ([3D], column blocks in `order` -- "kvq", or "qkv" for
    nn.MultiheadAttention's in_proj -- or, with order None, [D] of the q projection) or None; c_ref: the c_attn Parameter whose gradient
    is wanted (or None).  Only for gradients that live contiguously in the arena -- with or without a FoldQueue, so that a step computes
    the same bits whichever way its reductions run."""
    cs = _AttnCs()
    cs.fq = _fold() or K.ImmediateFold()                 # (no queue: gradients are consumed inside backward -- fold right behind the kernels)
    D = heads * 64
    gc = _sink(c_ref) if c_ref is not None else None
    use_b = gb is not None and gb.is_contiguous()
    cs.ns = K.attn_cs_slots(B, T, seg)
    if order and K.attn_cs_slots(B, S, seg, k_side=True) != cs.ns:
        use_b = False                                    # (self-attention: the same tiles on both sides -- anything else keeps the pass)
    if use_b:
        cs.bias_ws = torch.empty(cs.ns, len(order or "q") * D, dtype=torch.float32, device=dev)
        cs.bufs.update({n: cs.bias_ws[:, i * D:(i + 1) * D] for i, n in enumerate(order or "q")})
    if gc is not None and gc.is_contiguous():
        cs.c_ws = torch.empty(cs.ns, heads, dtype=torch.float32, device=dev)
        cs.bufs["c"] = cs.c_ws
    return cs


class _AttnBackward:
    """The attention backward of one call and what it leaves behind.  Constructing it launches the kernels: saved = (q, k, v, out, lse,
    bias, kpm, c_attn), cfg = (heads, scale, causal, seg, bias_shared), outs = the caller's (dq, dk, dv) views or None, c_ref = the c_attn
    Parameter whose gradient is wanted (or None), gb / order = the arena bias gradient the kernels' epilogues may serve (_attn_cs_begin),
    extra = further cs= buffers (CrossKVShared.dkv_cs' k= / v= slices), epilogue=False: no epilogue buffers at all.
    -> .grads (dq, dk, dv), .dbias (for autograd), .bias_part = (queue, partial rows, ns) of the bias column sums the epilogues
    produced (for _proj_backward) or None: the separate pass.  finish() -- AFTER the projections' launches -- completes c_attn."""

    def __init__(self, saved, cfg, dout, outs, need_dbias, c_ref, gb=None, order=None, extra=None, epilogue=True):
        q, k, v, out, lse, bias, kpm, c_attn = saved
        heads, scale, causal, seg, shared = cfg
        self.c_ref, self.dims = c_ref, (q.shape[0], heads, q.shape[1])
        # the bias gradients (column sums of dq / dk / dv) and the c_attn gradient come out of the backward kernels' epilogues as partial
        # rows for the FoldQueue when the gradients live in the arena: no pass over the d buffer, no c_attn_grad launch
        cs = self.cs = _attn_cs_begin(gb, c_ref, q.shape[0], q.shape[1], k.shape[1], seg, heads, q.device, order) if epilogue else _AttnCs()
        *self.grads, dbias, self.delta = K.attn_bwd(q, k, v, out, dout, lse, heads, scale, bias=bias, kpm=kpm, c_attn=c_attn, causal=causal,
                                                    need_dbias=need_dbias, seg=seg, bias_shared=shared,
                                                    dbias_dtype=_dbias_dtype(bias, shared), outs=outs, cs={**cs.bufs, **(extra or {})} or None)
        self.dbias = _shared_dbias(dbias, bias, shared)
        self.bias_part = (cs.fq, cs.bias_ws, cs.ns) if cs.bias_ws is not None else None

    def finish(self):
        """-> the c_attn gradient for autograd (None: not wanted, or it went to the arena)."""
        cs, dc = self.cs, None
        if cs.c_ws is not None:
            cs.fq.add(cs.c_ws, 0, _sink(self.c_ref), cs.c_ws.shape[1], cs.c_ws.shape[1], cs.ns, 1.0, True)
            _sink_done(self.c_ref)
        elif self.c_ref is not None:
            dc = _c_attn_grad(self.delta, self.c_ref, *self.dims)
        if cs.bufs:
            cs.fq.flush_if_large()
        return dc


def _packed(ws, arena_view):
    """Packed projection weight [sum(N_i), K] (or bias [sum N_i]): the arena view when the parameters are adjacent in
    the flat arena (zero copy), else a concatenated copy."""
    return arena_view if arena_view is not None else torch.cat([w.reshape(w.shape[0], -1) if w.dim() > 1 else w for w in ws])


def _slices(g, ws):
    """A fresh packed gradient's per-parameter slices, for autograd."""
    outs, o = [], 0
    for w in ws:
        n = w.shape[0]
        outs.append(g[o:o + n].view(w.shape))
        o += n
    return outs


def _proj_backward(d, x2, W, ws, bs, gw, gb, part, need):
    """Backward of a packed projection y = x2 W^T + b given d = dy [B, T, N] (contiguous): W [N, K] packs the weights `ws` row-wise, the
    biases `bs` likewise; gw / gb: their packed arena gradients (or None: fresh slices go back to autograd); part: _AttnBackward.bias_part;
    need = (dx, weights, biases) wanted.  One input-gradient GEMM, one weight-gradient product (through the layer's grouped launch when
    it goes to the arena) and the bias column sums: the registered partial rows, else one colsum.  Tells the sinks.
    -> dx [B, T, K] or None, [weight gradients], [bias gradients]."""
    d2 = d.view(-1, d.shape[-1])
    dx = K.gemm(d2, W, False, False).view(*d.shape[:-1], W.shape[1]) if need[0] else None
    gws, gbs = [None] * len(ws), [None] * len(bs)
    if need[1]:
        if gw is not None:
            _wgrad(d2, x2, gw, 1.0, *ws)
        else:
            gws = _slices(K.gemm(d2, x2, True, False), ws)
    if need[2]:
        if part is not None:
            fq, rows, ns = part
            fq.add(rows, 0, gb, rows.shape[1], rows.shape[1], ns, 1.0, True)
        elif gb is not None:
            K.colsum(d2, out=gb, accumulate=True, fold=_fold())
        else:
            gbs = _slices(K.colsum(d2, out_dtype=d2.dtype), bs)
        if gb is not None:
            for b in bs:
                _sink_done(b)
    return dx, gws, gbs


class FusedAttentionFn(torch.autograd.Function):
    """bf16 fused attention on [B,T,D] rows (csrc/attention.hip)."""

    @staticmethod
    def forward(ctx, q, k, v, bias, kpm, c_attn, heads, scale, causal, bias_shared=False):
        kpm, seg = _split_seg(kpm)
        out, lse = K.attn_fwd(q, k, v, heads, scale, bias=bias, kpm=kpm, c_attn=c_attn, causal=causal, seg=seg, bias_shared=bias_shared)
        ctx.save_for_backward(q, k, v, out, lse, bias, kpm, c_attn)
        ctx.c_ref = c_attn                                  # the Parameter object (carries the gradient sink)
        ctx.cfg = (heads, scale, causal, seg, bias_shared)
        return out

    @staticmethod
    def backward(ctx, dout):
        bias, c_attn = ctx.saved_tensors[5], ctx.saved_tensors[7]
        ab = _AttnBackward(ctx.saved_tensors, ctx.cfg, dout, None, bias is not None and ctx.needs_input_grad[3],
                           ctx.c_ref if (c_attn is not None and ctx.needs_input_grad[5]) else None, epilogue=False)
        return (*ab.grads, ab.dbias, None, ab.finish(), None, None, None, None)


class PackedSelfAttentionFn(torch.autograd.Function):
    """Self-attention core with ONE packed k|v|q projection (N = 3D) in front of the fused attention kernels
    (multihead_attention.py:199-346 up to, not including, out_proj).  The attention backward writes dk|dv|dq as column
    slices of one [B,T,3D] buffer (_AttnBackward), which then feeds one dgrad GEMM (K = 3D), one wgrad GEMM and one bias reduce
    (_proj_backward)."""

    @staticmethod
    def forward(ctx, x, wk, wv, wq, bk, bv, bq, bias, kpm, c_attn, heads, scale, causal, pack, bias_shared=False):
        B, T, D = x.shape
        W = _packed((wk, wv, wq), pack.get("w"))
        Bv = _packed((bk, bv, bq), pack.get("b"))
        x2d = x.view(B * T, D)
        kvq = K.gemm(x2d, W, False, True, bias=Bv).view(B, T, 3 * D)
        k, v, q = kvq[:, :, 0:D], kvq[:, :, D:2 * D], kvq[:, :, 2 * D:3 * D]
        kpm, seg = _split_seg(kpm)
        out, lse = K.attn_fwd(q, k, v, heads, scale, bias=bias, kpm=kpm, c_attn=c_attn, causal=causal, seg=seg, bias_shared=bias_shared)
        ctx.save_for_backward(x2d, kvq, out, lse, bias, kpm, c_attn, W)
        ctx.c_ref = c_attn
        ctx.params = (wk, wv, wq, bk, bv, bq)
        ctx.cfg = (heads, scale, causal, seg, bias_shared)
        ctx.pack = pack
        return out

    @staticmethod
    def backward(ctx, dout):
        x2d, kvq, out, lse, bias, kpm, c_attn, W = ctx.saved_tensors
        pack, D = ctx.pack, kvq.shape[2] // 3
        k, v, q = kvq[:, :, 0:D], kvq[:, :, D:2 * D], kvq[:, :, 2 * D:3 * D]
        dkvq = torch.empty_like(kvq)                                   # (ragged mode: the kernels zero the filler rows)
        ab = _AttnBackward((q, k, v, out, lse, bias, kpm, c_attn), ctx.cfg, dout, (dkvq[:, :, 2 * D:3 * D], dkvq[:, :, 0:D], dkvq[:, :, D:2 * D]),
                           bias is not None and ctx.needs_input_grad[7], ctx.c_ref if (c_attn is not None and ctx.needs_input_grad[9]) else None,
                           gb=pack.get("gb"), order="kvq")
        dx, gws, gbs = _proj_backward(dkvq, x2d, W, ctx.params[:3], ctx.params[3:], pack.get("gw"), pack.get("gb"), ab.bias_part,
                                      (ctx.needs_input_grad[0], True, True))
        return (dx, *gws, *gbs, ab.dbias, None, ab.finish(), None, None, None, None, None)


class InProjSelfAttentionFn(torch.autograd.Function):
    """Self-attention core over nn.MultiheadAttention's single packed parameter pair in_proj_weight [3D, D] / in_proj_bias [3D] (q|k|v
    row blocks, read in place: no reorder, no copy) in front of the fused attention kernels: one N = 3D GEMM, attention on the column
    slices (no bias, no mask, no c_attn).  The backward is PackedSelfAttentionFn's, the "pack" being the parameter pair itself in
    column order "qkv".  16-bit operands, head_dim 64 (module/vit.py keeps everything else on ops.linear + ops.attention)."""

    @staticmethod
    def forward(ctx, x, w, b, heads, scale):
        B, T, D = x.shape
        x2d = x.view(B * T, D)
        qkv = K.gemm(x2d, w, False, True, bias=b).view(B, T, 3 * D)
        out, lse = K.attn_fwd(qkv[:, :, 0:D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:3 * D], heads, scale)
        ctx.save_for_backward(x2d, qkv, out, lse, w)
        ctx.bias_ref = b
        ctx.cfg = (heads, scale, False, None, False)
        return out

    @staticmethod
    def backward(ctx, dout):
        x2d, qkv, out, lse, w = ctx.saved_tensors
        b, D = ctx.bias_ref, qkv.shape[2] // 3
        gb = _sink(b) if ctx.needs_input_grad[2] else None
        dqkv = torch.empty_like(qkv)
        ab = _AttnBackward((qkv[:, :, 0:D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:3 * D], out, lse, None, None, None), ctx.cfg, dout,
                           (dqkv[:, :, 0:D], dqkv[:, :, D:2 * D], dqkv[:, :, 2 * D:3 * D]), False, None, gb=gb, order="qkv")
        dx, (dw,), (db,) = _proj_backward(dqkv, x2d, w, (w,), (b,), _sink(w), gb, ab.bias_part, ctx.needs_input_grad)
        ab.finish()
        return dx, dw, db, None, None


def in_proj_self_attention_ok(x, heads):
    """Does InProjSelfAttentionFn take this input (16-bit operands, head_dim 64)?"""
    return x.dtype in (torch.bfloat16, torch.float16) and x.shape[-1] == heads * 64


def in_proj_self_attention(x, in_proj_weight, in_proj_bias, heads):
    """Self-attention core of nn.MultiheadAttention(D, heads) on batch-major rows x [B,T,D], up to (not including) out_proj.  The
    fused path where in_proj_self_attention_ok; otherwise the unfused tier: three ops.linear over the parameter's row blocks (views)
    and ops.attention."""
    B, T, D = x.shape
    scale = (D // heads) ** -0.5
    if in_proj_self_attention_ok(x, heads):
        return InProjSelfAttentionFn.apply(x.contiguous(), in_proj_weight, in_proj_bias, heads, scale)
    q, k, v = (linear(x, in_proj_weight[i * D:(i + 1) * D], in_proj_bias[i * D:(i + 1) * D]) for i in range(3))
    return attention(q, k, v, heads, scale)[0]


class CrossKVShared:
    """The k|v projections of the encoder output for ALL decoder layers as one GEMM (multihead_attention.py:203-211 runs k_proj and
    v_proj of every layer's encoder_attn on the same encoder_out): kv_all = enc W_all^T + b_all, [rows, layers * 2D], layer l's k | v
    in columns [l*2D, (l+1)*2D).  Backward: every layer's attention backward writes its dk | dv slice of ONE buffer; the layer-0 node
    -- the last cross-attention backward to run, by data dependence -- then issues the single input-gradient GEMM (K = layers * 2D)
    for the encoder output, queues the single weight-gradient product and the bias column sums.  pack: trainer.FlatParams' arena
    views of the packed weights (the parameters are adjacent there)."""

    def __init__(self, enc_rows, pack):
        self.pack, self.L, self.D = pack, pack["layers"], pack["D"]
        self.enc2d = enc_rows
        self.kv_all = K.gemm(enc_rows, pack["w"], False, True, bias=pack["b"])          # [rows, L * 2D]
        self.dkv_all = None
        self.cs_all = None                                  # fp32 partial rows of colsum(dkv_all), written by the dK/dV kernels (dkv_cs)
        self.done = 0
        self.users = set()                                  # layers whose fused attention reads its slice (registered in forward)

    def use(self, layer):
        self.users.add(layer)

    def kv(self, layer, B, S):
        lo = layer * 2 * self.D
        return self.kv_all[:, lo:lo + 2 * self.D].view(B, S, 2 * self.D)               # (row stride L * 2D: a column slice)

    def dkv(self, layer, B, S):
        if self.dkv_all is None:
            self.dkv_all = torch.empty_like(self.kv_all)
        lo = layer * 2 * self.D
        return self.dkv_all[:, lo:lo + 2 * self.D].view(B, S, 2 * self.D)

    def dkv_cs(self, layer, ns):
        """Layer `layer`'s k= / v= column slices (kernels.attn_bwd cs=) of the stack-wide partial rows of colsum(dkv_all) [ns, L * 2D] (fp32) -- every layer's
        dK/dV kernel writes its own slice, finish() registers ONE fold -- or None when the bias gradient takes the separate pass."""
        gb = self.pack.get("gb")
        if len(self.users) != self.L or gb is None or not gb.is_contiguous():
            return None
        if self.cs_all is None:
            self.cs_all = torch.empty(ns, self.L * 2 * self.D, dtype=torch.float32, device=self.kv_all.device)
        assert self.cs_all.shape[0] == ns
        lo = layer * 2 * self.D
        return {"k": self.cs_all[:, lo:lo + self.D], "v": self.cs_all[:, lo + self.D:lo + 2 * self.D]}

    def finish(self, need_dx):
        """After the last participating layer's slice has been written: d enc, d W_all, d b_all.  A layer that did not take part
        (it needed the attention weights: exact tier, own projection, own gradients) contributes zeros here."""
        assert self.done == len(self.users), (self.done, sorted(self.users))
        p = self.pack
        for layer in range(self.L):
            if layer not in self.users:
                self.dkv_all[:, layer * 2 * self.D:(layer + 1) * 2 * self.D].zero_()
        dx = K.gemm(self.dkv_all, p["w"], False, False) if need_dx else None
        L, D = self.L, self.D
        if len(self.users) == L:                            # every layer took part: ONE weight-gradient product, ONE column sum
            # (a filler: the encoder layers' groups, whose backward starts right behind this node, take it along in their idle CUs)
            _wgrad(self.dkv_all, self.enc2d, p["gw"], 1.0, *p["params"][:2 * L], filler=True)
            fq = _fold()
            if self.cs_all is not None:
                fq2 = fq or K.ImmediateFold()
                fq2.add(self.cs_all, 0, p["gb"], L * 2 * D, L * 2 * D, self.cs_all.shape[0], 1.0, True)
                fq2.flush_if_large()
            else:
                K.colsum(self.dkv_all, out=p["gb"], accumulate=True, out_dtype=self.dkv_all.dtype, fold=fq)
        else:
            # a layer that kept its own projection already owns (and may already be all-reducing) its gradient rows: touch only
            # the participating layers' slices
            for layer in sorted(self.users):
                sl = slice(layer * 2 * D, (layer + 1) * 2 * D)
                _wgrad(self.dkv_all[:, sl], self.enc2d, p["gw"][sl], 1.0, *p["params"][2 * layer:2 * layer + 2])
                K.colsum(self.dkv_all[:, sl], out=p["gb"][sl], accumulate=True, out_dtype=self.dkv_all.dtype, fold=_fold())
        for layer in sorted(self.users):                    # (a non-participating layer's own backward reports its parameters)
            for b in p["params"][2 * L + 2 * layer:2 * L + 2 * layer + 2]:
                _sink_done(b)
        return dx


class PackedCrossAttentionFn(torch.autograd.Function):
    """Encoder-decoder attention core: q projection from the decoder stream, ONE packed k|v projection (N = 2D) from the
    encoder output (multihead_attention.py:203-211)."""

    @staticmethod
    def forward(ctx, xq, xkv, wk, wv, wq, bk, bv, bq, bias, kpm, c_attn, heads, scale, pack, bias_shared=False, kv_all=None, layer=0):
        """kv_all (CrossKVShared) / layer: the k|v rows come from the stack-wide projection; xkv is then only an input of layer 0 (so
        that its node can hand the encoder output's gradient back), None elsewhere."""
        B, T, D = xq.shape
        xq2 = xq.view(B * T, D)
        q = K.gemm(xq2, wq, False, True, bias=bq).view(B, T, D)
        ctx.kv_all, ctx.layer = kv_all, layer
        if kv_all is not None:
            S = kv_all.kv_all.shape[0] // B
            W = xkv2 = None
            kv = kv_all.kv(layer, B, S)
            kv_all.use(layer)
        else:
            S = xkv.shape[1]
            W = _packed((wk, wv), pack.get("w"))
            Bv = _packed((bk, bv), pack.get("b"))
            xkv2 = xkv.view(B * S, D)
            kv = K.gemm(xkv2, W, False, True, bias=Bv).view(B, S, 2 * D)
        k, v = kv[:, :, 0:D], kv[:, :, D:2 * D]
        kpm, seg = _split_seg(kpm)
        out, lse = K.attn_fwd(q, k, v, heads, scale, bias=bias, kpm=kpm, c_attn=c_attn, causal=False, seg=seg, bias_shared=bias_shared)
        ctx.save_for_backward(xq2, xkv2, q, (kv if kv_all is None else None), out, lse, bias, kpm, c_attn, W)
        ctx.c_ref = c_attn
        ctx.params = (wk, wv, wq, bk, bv, bq)
        ctx.cfg = (heads, scale, False, seg, bias_shared)
        ctx.pack = pack
        return out

    @staticmethod
    def backward(ctx, dout):
        xq2, xkv2, q, kv, out, lse, bias, kpm, c_attn, W = ctx.saved_tensors
        wk, wv, wq, bk, bv, bq = ctx.params
        B, T, D = q.shape
        shared_kv, kv_cs = ctx.kv_all, None
        if shared_kv is not None:
            # the k | v side of a stack-wide projection: the layer's slice of the ONE d buffer, its bias column sums into CrossKVShared's
            # partial rows, folded once by finish()
            S = shared_kv.kv_all.shape[0] // B
            kv, dkv = shared_kv.kv(ctx.layer, B, S), shared_kv.dkv(ctx.layer, B, S)
            kv_cs = shared_kv.dkv_cs(ctx.layer, K.attn_cs_slots(B, S, ctx.cfg[3], k_side=True))
        else:
            dkv = torch.empty_like(kv)
        dq = torch.empty_like(q)                                       # (ragged mode: the kernels zero the filler rows)
        ab = _AttnBackward((q, kv[:, :, 0:D], kv[:, :, D:2 * D], out, lse, bias, kpm, c_attn), ctx.cfg, dout,
                           (dq, dkv[:, :, 0:D], dkv[:, :, D:2 * D]), bias is not None and ctx.needs_input_grad[8],
                           ctx.c_ref if (c_attn is not None and ctx.needs_input_grad[10]) else None, gb=_sink(bq), extra=kv_cs)
        dxq, (gq,), (gbq,) = _proj_backward(dq, xq2, wq, (wq,), (bq,), _sink(wq), _sink(bq), ab.bias_part,
                                            (ctx.needs_input_grad[0], True, True))
        if shared_kv is not None:
            # the slice is written; layer 0 -- the last cross-attention backward of the stack -- closes the shared projection
            shared_kv.done += 1
            dxkv, gws, gbs = None, [None, None], [None, None]
            if ctx.layer == min(shared_kv.users):
                dx2 = shared_kv.finish(ctx.needs_input_grad[1])
                dxkv = dx2.view(B, S, D) if dx2 is not None else None
        else:
            dxkv, gws, gbs = _proj_backward(dkv, xkv2, W, (wk, wv), (bk, bv), ctx.pack.get("gw"), ctx.pack.get("gb"), None,
                                            (ctx.needs_input_grad[1], True, True))
        return (dxq, dxkv, *gws, gq, *gbs, gbq, ab.dbias, None, ab.finish(), None, None, None, None, None, None)


class UnfusedAttentionFn(torch.autograd.Function):
    """Exact-tier attention (any dtype): scores and probabilities are materialised, every product is a per-(batch, head)
    GEMM on the [B,T,D] rows.  Used for fp32 parity, need_weights and attention dropout.  Returns (out, probs)."""

    @staticmethod
    def forward(ctx, q, k, v, bias, kpm, c_attn, heads, scale, causal, dropout_p):
        B, T, D = q.shape
        S = k.shape[1]
        hd = D // heads
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        scores = torch.empty(B * heads, T, S, dtype=q.dtype, device=q.device)
        K.gemm_heads(q, k, scores, T, S, hd, False, True, D, D, S, B, heads, hd, T * D, hd, S * D, T * S, heads * T * S)
        p = K.attn_softmax(scores, bias, kpm, scale, heads, causal)
        pd = p
        seed = off = 0
        base = None
        if dropout_p > 0:
            seed, off, base = _Rng.reserve(p.numel(), p.device)
            pd = K.dropout_add(p, None, dropout_p, seed, off, base)
        o = torch.empty(B, T, D, dtype=q.dtype, device=q.device)
        K.gemm_heads(pd, v, o, T, hd, S, False, False, S, D, D, B, heads, T * S, heads * T * S, hd, S * D, hd, T * D)
        out = _scale_heads(o, c_attn, heads) if c_attn is not None else o
        ctx.save_for_backward(q, k, v, p, o, c_attn)
        ctx.cfg = (heads, scale, dropout_p, seed, off, base)
        return out, p

    @staticmethod
    def backward(ctx, dout, dp_unused):
        q, k, v, p, o, c_attn = ctx.saved_tensors
        heads, scale, dropout_p, seed, off, base = ctx.cfg
        B, T, D = q.shape
        S = k.shape[1]
        hd = D // heads
        dout = dout.contiguous()
        dc = None
        do = dout
        if c_attn is not None:
            prod = K.mul(dout, o)                                             # d c[h] = sum_{b,t,d} dout * (PV)
            dc = K.colsum(K.colsum(prod.view(-1, D)).view(heads, hd).t().contiguous()).to(c_attn.dtype)
            do = _scale_heads(dout, c_attn, heads)
        pd = p
        if dropout_p > 0:
            pd = K.dropout_add(p, None, dropout_p, seed, off, base)
        dv = torch.empty_like(v)
        K.gemm_heads(pd, do, dv, S, hd, T, True, False, S, D, D, B, heads, T * S, heads * T * S, hd, T * D, hd, S * D)
        dpd = torch.empty_like(p)
        K.gemm_heads(do, v, dpd, T, S, hd, False, True, D, D, S, B, heads, hd, T * D, hd, S * D, T * S, heads * T * S)
        if dropout_p > 0:
            dpd = K.dropout_bwd(dpd, dropout_p, seed, off, base)
        ds = K.scaled_softmax_bwd(dpd, p, 1.0)                                  # dS wrt (scale*qk + bias)
        dq = torch.empty_like(q)
        K.gemm_heads(ds, k, dq, T, hd, S, False, False, S, D, D, B, heads, T * S, heads * T * S, hd, S * D, hd, T * D,
                     alpha=scale)
        dk = torch.empty_like(k)
        K.gemm_heads(ds, q, dk, S, hd, T, True, False, S, D, D, B, heads, T * S, heads * T * S, hd, T * D, hd, S * D,
                     alpha=scale)
        dbias = ds if ctx.needs_input_grad[3] else None
        return dq, dk, dv, dbias, None, dc, None, None, None, None


def _scale_heads(x, c_attn, heads):
    """x[b,t,h,:] * c[h]  (multihead_attention.py:342-345) with the row-vector multiply kernel."""
    B, T, D = x.shape
    vec = c_attn.to(x.dtype).view(heads, 1).expand(heads, D // heads).reshape(-1)
    return K.mul_rowvec(x.view(-1, D), vec).view(B, T, D)


class SharedBias:
    """A position bias that is the same for every sample: t = [A, Tb, Sb] (the reference's [B, A, T, T] / [B*A, T, S] tensor is B
    copies of it).  MultiheadAttention hands t to the fused kernels (ofa_attn_sbias_*: indexed by the position inside the sample,
    gradient summed over the batch in-kernel) or expands it for the exact tier."""
    __slots__ = ("t", "swz")

    def __init__(self, t, swz=None):
        assert t.dim() == 3
        self.t = t
        self.swz = swz               # (row image, column image) of t for the fused kernels (K.bias_build), or None: built per call

    def shared_arg(self):
        """What the attention Functions take as `bias_shared`: the swizzled images when they exist, else True."""
        return self.swz if self.swz is not None else True

    @staticmethod
    def of(t):
        """A shared bias that needs no assembly (the decoder's cross-attention abs-pos bias): t [A, Tt, Ts] + its swizzled images."""
        swz = None
        if t.is_cuda and t.dtype in (torch.bfloat16, torch.float16):
            swz = K.bias_build(t.detach(), want_out=False)[1]
        return SharedBias(t, swz)


def expand_shared_bias(bias, B, T, S):
    """[A, Tb, Sb] shared position bias -> the reference's dense [B*A, T, S] (exact tier / attention-weight outputs); autograd
    reduces the expand."""
    A = bias.shape[0]
    return bias[:, :T, :S].unsqueeze(0).expand(B, A, T, S).reshape(B * A, T, S)


def attention(q, k, v, heads, scale, bias=None, key_padding_mask=None, c_attn=None, causal=False, dropout_p=0.0,
              need_weights=False):
    """Attention core on [B,T,D] rows.  Returns (out [B,T,D], probs [B*heads,T,S] or None)."""
    fused_ok = (q.dtype in (torch.bfloat16, torch.float16) and q.shape[-1] // heads == 64 and dropout_p == 0.0 and not need_weights)
    if bias is not None and bias.dtype != q.dtype:
        bias = bias.to(q.dtype)
    shared = bias is not None and bias.dim() == 3 and bias.shape[0] == heads          # [A, T, S]: one bias for every sample
    if fused_ok:
        return FusedAttentionFn.apply(q, k, v, bias, key_padding_mask, c_attn, heads, scale, causal, shared), None
    if shared:
        if key_padding_mask is not None and not torch.is_tensor(key_padding_mask):
            raise NotImplementedError("packed (ragged) batches run on the fused attention kernels only")
        bias = expand_shared_bias(bias, q.shape[0], q.shape[1], k.shape[1])
    if key_padding_mask is not None and not torch.is_tensor(key_padding_mask):
        raise NotImplementedError("packed (ragged) batches run on the fused bf16 attention kernels only "
                                  "(bf16, head_dim 64, no attention dropout, no attention-weight output)")
    out, p = UnfusedAttentionFn.apply(q, k, v, bias, key_padding_mask, c_attn, heads, scale, causal, dropout_p)
    return out, p


# ---------------------------------------------------------------------------------------------- position biases
class HeadsMatmulNTFn(torch.autograd.Function):
    """out[b,a] = x_{b,a} y_{b,a}^T for x [B,T,D], y [B,S,D] rows split into `heads` column groups -> [B,A,T,S]
    (abs-pos bias, adaptor/general.py:223-243; cross abs-pos bias, model/transformer.py:280-299)."""

    @staticmethod
    def forward(ctx, x, y, heads, alpha):
        x, y = x.contiguous(), y.contiguous()
        B, T, D = x.shape
        S = y.shape[1]
        hd = D // heads
        out = torch.empty(B, heads, T, S, dtype=x.dtype, device=x.device)
        K.gemm_heads(x, y, out, T, S, hd, False, True, D, D, S, B, heads, hd, T * D, hd, S * D, T * S, heads * T * S,
                     alpha=alpha)
        ctx.save_for_backward(x, y)
        ctx.heads, ctx.alpha = heads, alpha
        return out

    @staticmethod
    def backward(ctx, dout):
        x, y = ctx.saved_tensors
        heads, alpha = ctx.heads, ctx.alpha
        B, T, D = x.shape
        S = y.shape[1]
        hd = D // heads
        dout = dout.contiguous()
        dx = torch.empty_like(x)
        dy = torch.empty_like(y)
        K.gemm_heads(dout, y, dx, T, hd, S, False, False, S, D, D, B, heads, T * S, heads * T * S, hd, S * D, hd, T * D,
                     alpha=alpha)
        K.gemm_heads(dout, x, dy, S, hd, T, True, False, S, D, D, B, heads, T * S, heads * T * S, hd, T * D, hd, S * D,
                     alpha=alpha)
        return dx, dy, None, None


def heads_matmul_nt(x, y, heads, alpha=1.0):
    return HeadsMatmulNTFn.apply(x, y, heads, alpha)


class OuterRelPos:
    """The rel-pos values of a video slot, un-materialised: value(i, j) = frames[i // P][j // P] + patches[i % P][j % P]
    (frames [F, F, A]: frame-level table lookups, patches [P, P, A]: the image adaptor's; video_image_sequence.py:187-204 adds the
    two broadcast views into an [F P, F P, A] tensor per layer -- 59 MB at cfg-4 -- and autograd reduces its gradient twice).  The bias
    assembly (BiasAssembleFn / ofa_bias_build) reads the two tables, the gradient kernels (ofa_bias_outer_grad) sum straight into them."""
    __slots__ = ("frames", "patches")

    def __init__(self, frames, patches):
        assert frames.dim() == 3 and patches.dim() == 3 and frames.shape[-1] == patches.shape[-1]
        self.frames, self.patches = frames, patches

    @property
    def n(self):
        return self.frames.shape[0] * self.patches.shape[0]

    def dense(self):
        Fr, P, A = self.frames.shape[0], self.patches.shape[0], self.frames.shape[-1]
        return (self.frames.view(Fr, 1, Fr, 1, A) + self.patches.view(1, P, 1, P, A)).reshape(Fr * P, Fr * P, A)


class LazyRelPosBias:
    """What an adaptor returns in `self_attn_bias` instead of the reference's [B, A, T, T] expand view when the values are an
    OuterRelPos: the general adaptor's assembly takes `.values`; `.materialize()` is the reference's tensor."""
    __slots__ = ("values", "batch_size")

    def __init__(self, values, batch_size):
        self.values, self.batch_size = values, batch_size

    def materialize(self):
        return self.values.dense().unsqueeze(0).expand(self.batch_size, -1, -1, -1).permute([0, 3, 1, 2])


class FanOutFn(torch.autograd.Function):
    """n views of one tensor for n consumers whose gradients are summed in ONE launch (K.add_n: fp32 accumulation, one rounding) when
    the last of them arrives, instead of autograd's n - 1 pairwise adds (5 x 61 MB per stack for the abs-position bias at cfg-4)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        gs = [g for g in grads if g is not None]
        if not gs:
            return None, None
        # ofa_add_n takes contiguous, 16-byte aligned inputs of ONE dtype; a gradient that is a view at an odd offset, strided, or of
        # another dtype (an fp32 gradient from the exact-tier attention path) takes autograd's own pairwise adds instead of raising
        # in the middle of backward
        fast = all(g.dtype == gs[0].dtype and g.is_contiguous() and g.data_ptr() % 16 == 0 and g.shape == gs[0].shape for g in gs)
        if not fast:
            out = gs[0]
            for g in gs[1:]:
                out = out + g.to(out.dtype) if g.dtype != out.dtype else out + g
            return out, None
        out, i = gs[0], 1
        while i < len(gs):                                  # (16 inputs per launch: the running sum + the next 15)
            out = K.add_n([out] + gs[i:i + 15])
            i += 15
        return out, None


def fan_out(x, n):
    """[x_0 .. x_{n-1}], all views of x: hand x_l to consumer l (layer l of a stack)."""
    if n <= 1 or not (torch.is_grad_enabled() and x.requires_grad and x.is_cuda):
        return [x] * n
    return list(FanOutFn.apply(x, n))


def fan_out_bias(bias, n):
    """A stack-wide attention bias (None, a dense tensor or a SharedBias) as one object per layer, see fan_out."""
    if bias is None or bias is False:
        return [bias] * n
    if isinstance(bias, SharedBias):
        return [SharedBias(t, bias.swz) for t in fan_out(bias.t, n)]
    return fan_out(bias, n)


class BiasAssembleFn(torch.autograd.Function):
    """bias_l = abs.clone(); bias_l[:, :, s:e, s:e] += values_k for each slot k (adaptor/general.py:270-280).
    kinds[k]: None (no values), "dense" (one tensor [n_k, n_k, A]: the un-expanded rel-pos values), "outer" (two tensors, frames
    [F,F,A] and patches [P,P,A]: an OuterRelPos) or "batch" (one tensor [B, A, n_k, n_k]: a custom adaptor's own per-sample bias,
    adaptor/base.py:183-189 -- only in the dense [B, A, T, T] form); `tensors` holds them in slot order."""

    @staticmethod
    def forward(ctx, abs_bias, starts, kinds, *tensors):
        it = iter(tensors)
        values = [None if k is None else ((next(it), next(it)) if k == "outer" else next(it)) for k in kinds]
        blocks = []
        for s, k, v in zip(starts, kinds, values):
            if k is None:
                blocks.append(None)
            elif k == "outer":
                blocks.append((s, v[0].shape[0], v[1].shape[0], v[0].dtype))
            elif k == "batch":
                blocks.append(("batch", s, v.shape[-1], v.dtype))
            else:
                blocks.append((s, v.shape[0], v.dtype))
        ctx.blocks = blocks
        ctx.set_materialize_grads(False)         # (the two image outputs never carry a gradient: no zero tensors for them)
        if abs_bias.shape[0] == 1 and abs_bias.is_cuda and abs_bias.dtype in (torch.bfloat16, torch.float16) and "batch" not in kinds:
            # the batch-shared form: ONE launch assembles the layer's matrix and writes the two swizzled images the fused attention
            # kernels read (ofa_bias_build) -- was a clone + one block add per slot
            out, swz = K.bias_build(abs_bias[0], starts, values)
            ctx.mark_non_differentiable(*swz)
            return out.unsqueeze(0), swz[0], swz[1]
        out = abs_bias.clone(memory_format=torch.contiguous_format)
        for s, k, v in zip(starts, kinds, values):
            if v is None:
                continue
            if k == "batch":
                assert v.shape[0] == out.shape[0] and v.shape[1] == out.shape[1] and v.shape[2] == v.shape[3], \
                    f"per-sample self_attn_bias {tuple(v.shape)} does not fit the layer bias {tuple(out.shape)}"
                K.bias_block_add_batch_(out, v.to(out.dtype), s)
                continue
            if k == "outer":
                v = OuterRelPos(*v).dense()
            K.bias_block_add_(out, v.to(out.dtype), s)
        return out, None, None

    @staticmethod
    def backward(ctx, dout, _dr=None, _dc=None):
        if dout is None:
            return (None, None, None) + (None,) * sum(0 if b is None else (2 if (len(b) == 4 and b[0] != "batch") else 1) for b in ctx.blocks)
        grads = []
        for blk in ctx.blocks:
            if blk is None:
                continue
            if blk[0] == "batch":                               # per-sample slot: its block of the gradient, as it is
                _, s, n, dt = blk
                grads.append(K.bias_block_slice(dout, s, n).to(dt))
            elif len(blk) == 4:                                 # outer slot: sum the block straight into the two tables
                s, Fr, P, dt = blk
                if dout.shape[0] == 1 and dout.is_cuda:
                    dvf, dvi = K.bias_outer_grad(dout, s, Fr, P)
                else:
                    d = K.bias_block_grad(dout, s, Fr * P).view(Fr, P, Fr, P, -1).float()
                    dvf, dvi = d.sum((1, 3)), d.sum((0, 2))
                grads += [dvf.to(dt), dvi.to(dt)]
            else:
                s, n, dt = blk
                grads.append(K.bias_block_grad(dout, s, n).to(dt))
        return (dout, None, None, *grads)


class MulRowvecFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, vec):
        ctx.save_for_backward(a, vec)
        return K.mul_rowvec(a, vec)

    @staticmethod
    def backward(ctx, dy):
        a, vec = ctx.saved_tensors
        return K.mul_rowvec(dy, vec), K.colsum(K.mul(dy, a), out_dtype=vec.dtype)


def mul_rowvec(a, vec):
    a2d, restore = rows_view(a)
    return restore(MulRowvecFn.apply(a2d, vec))


class ScaleFn(torch.autograd.Function):
    """y = fwd * x, dx = bwd * dy (constants): `embed_scale * embed` and the gradient-only rescale
    `embed * a + embed.detach() * (1 - a)` of the adaptor post-hook (adaptor/base.py:168, 174-176) on the row-vector multiply kernel."""
    _scalars = {}

    @classmethod
    def _scalar(cls, value, like):
        """The factor as ONE fp32 element on the device: the multiply runs in fp32 and rounds once, as the reference's
        `bf16 tensor * Python scalar` does (fp32 opmath).  A factor stored in the activation dtype would round first -- sqrt(768) =
        27.7128 becomes 27.75 in bf16, +0.13 % on every embedding."""
        key = (float(value), like.device)
        v = cls._scalars.get(key)
        if v is None:
            v = cls._scalars[key] = torch.full((1,), float(value), dtype=torch.float32, device=like.device)
        return v

    @staticmethod
    def forward(ctx, x2d, fwd, bwd):
        ctx.bwd = bwd
        if fwd == 1.0 or x2d.shape[0] == 0:
            return x2d.view_as(x2d)
        return K.scale_row_groups(x2d, ScaleFn._scalar(fwd, x2d), x2d.shape[0])

    @staticmethod
    def backward(ctx, dy):
        if ctx.bwd == 1.0 or dy.shape[0] == 0:
            return dy, None, None
        dy = dy.contiguous()
        return K.scale_row_groups(dy, ScaleFn._scalar(ctx.bwd, dy), dy.shape[0]), None, None


def scale(x, fwd=1.0, bwd=None):
    """fwd * x with gradient bwd * dy (bwd defaults to fwd: a plain scalar multiply)."""
    bwd = fwd if bwd is None else bwd
    if fwd == 1.0 and bwd == 1.0:
        return x
    x2d, restore = rows_view(x)
    return restore(ScaleFn.apply(x2d, float(fwd), float(bwd)))


# ---------------------------------------------------------------------------------------------- patch embedding
class PatchEmbedFn(torch.autograd.Function):
    """Conv2d(C, D, kernel=stride=p) as im2col + MFMA GEMM, with the class token in place (adaptor/image_patch_embed.py:59-73).
    img [B,C,H,W], weight [D,C,p,p], bias [D], cls [1,1,D] or None -> [B, (1 +) (H/p)*(W/p), D].  With a class token the im2col matrix
    carries one all-zero row in front of every sample's patches: ONE GEMM writes the [B, 1 + N, D] result (the reference concatenates),
    the class-token rows are then overwritten with the token, and in backward the weight gradient is ONE contraction over the same rows
    (a zero row contributes nothing) of the incoming gradient as it is -- no slice, no copy.  The image gets no gradient (an input)."""

    @staticmethod
    def forward(ctx, img, weight, bias, cls, p):
        B, C, H, W = img.shape
        D = weight.shape[0]
        Kc = C * p * p
        Kpad = (Kc + 7) // 8 * 8
        lead = 0 if cls is None else 1
        col = K.im2col_patch(img.to(weight.dtype), p, Kpad, lead)
        wp = weight.reshape(D, Kc)
        if Kpad != Kc:                                       # k-major operand rows are whole 16-byte vectors: pad the weight's K
            wp2 = getattr(weight, "_ofa_kpad", None)         # (the zero tail is written once; every step copies the live columns)
            if wp2 is None or wp2.shape != (D, Kpad) or wp2.dtype != weight.dtype or wp2.device != weight.device:
                wp2 = weight.new_zeros(D, Kpad)
                if not (weight.is_cuda and torch.cuda.is_current_stream_capturing()):
                    weight._ofa_kpad = wp2
            wp2[:, :Kc].copy_(wp.detach())
            wp = wp2
        out = K.gemm(col, wp, False, True, bias=bias).view(B, lead + (H // p) * (W // p), D)
        if cls is not None:
            out[:, 0, :] = cls.reshape(1, D).to(out.dtype)   # (the GEMM left the bias there)
        ctx.save_for_backward(col)
        ctx.meta = (weight.shape, Kc, Kpad, lead)
        ctx.refs = (weight, bias, cls)
        return out

    @staticmethod
    def backward(ctx, dout):
        (col,) = ctx.saved_tensors
        wshape, Kc, Kpad, lead = ctx.meta
        weight, bias, cls = ctx.refs
        B, T, D = dout.shape
        d2 = dout.reshape(B * T, D)
        d2 = d2 if d2.is_contiguous() else d2.contiguous()
        dw = db = dcls = None
        gw = _sink(weight)
        if gw is not None and gw.is_contiguous() and Kc % 4 == 0:
            K.gemm(d2, col[:, :Kc], True, False, out=gw.view(wshape[0], Kc), accumulate=True)   # straight onto the arena gradient (ldb = Kpad)
            _sink_done(weight)
        else:
            dw = K.gemm(d2, col, True, False)[:, :Kc].reshape(wshape)
        first = dout[:, 0, :] if lead else None              # [B, D] rows (B * T * D apart): the class-token positions
        if cls is not None:
            gc = _sink(cls)
            if gc is not None:
                K.colsum(first, out=gc.view(-1), accumulate=True, fold=_edge_fold(), same_bits=True)
                _sink_done(cls)
            else:
                dcls = K.colsum(first, out_dtype=dout.dtype).view(cls.shape)
        if bias is not None:
            gb = _sink(bias)
            if gb is not None:
                K.colsum(d2, out=gb, accumulate=True, fold=_edge_fold(), same_bits=True)
                if lead:
                    # the class-token rows never saw the bias (a second contribution to gb: the queue keeps it out of the first one's launch)
                    K.colsum(first, alpha=-1.0, out=gb, accumulate=True, fold=_edge_fold(), same_bits=True)
                _sink_done(bias)
            else:
                db = K.colsum(d2, out_dtype=dout.dtype)
                if lead:
                    db = db - K.colsum(first, out_dtype=dout.dtype)
        return None, dw, db, dcls, None


def patch_embed(img, weight, bias, p, cls_token=None):
    """[B, C, H, W] -> [B, N, D], or [B, 1 + N, D] with `cls_token` [1, 1, D] in front of every sample's patches."""
    return PatchEmbedFn.apply(img, weight, bias, cls_token, p)


# ---------------------------------------------------------------------------------------------- criterion
def _ce_rows(logits):
    """[..., V] logits -> [rows, V] view whose row stride is a multiple of the 16-byte vector width (copy only if needed)."""
    V = logits.shape[-1]
    if logits.is_contiguous():
        l2d = logits.reshape(-1, V)
    else:
        try:
            l2d = logits.view(-1, V)                       # a padded-stride view of row storage: no copy
        except RuntimeError:
            l2d = logits.contiguous().view(-1, V)          # a transposed [T, B, V] layout (op-by-op layer stacks)
    if l2d.stride(1) != 1 or l2d.stride(0) % (4 if l2d.dtype == torch.float32 else 8) != 0:
        pad = (-V) % 8
        store = torch.zeros(l2d.shape[0], V + pad, dtype=l2d.dtype, device=l2d.device)
        store[:, :V].copy_(l2d)
        l2d = store[:, :V]
    return l2d


def _range(constraint_range):
    return constraint_range if constraint_range is not None else (-1, -1)


def _criterion_rows(who, logits, target, constraint_range=None, constraint_masks=None, nodes=None):
    """What every criterion over [..., V] logits starts with -> (the [rows, V] view, the flat target, cs, ce, the [rows, V] masks or
    None, the nodes as int32 [rows] on the logits' device or None)."""
    V = logits.shape[-1]
    l2d = _ce_rows(logits)
    t = target.reshape(-1).contiguous()
    cm = constraint_masks.reshape(-1, V).contiguous() if constraint_masks is not None else None
    nd = None
    if nodes is not None:
        nd = nodes.reshape(-1).to(device=l2d.device, dtype=torch.int32).contiguous()
        if nd.numel() != l2d.shape[0]:
            raise ValueError(f"{who}: {nd.numel()} nodes for {l2d.shape[0]} rows")
    return (l2d, t, *_range(constraint_range), cm, nd)


def _drop_rank(row_loss, valid, drop_worst_ratio):
    """The drop-worst ranking on row_loss, on the device (a stable sort, no host sync) -> (keep: the rows that stay, their number k)."""
    n = valid.sum()
    k = (n.double() * (1 - drop_worst_ratio)).floor().long()                        # int(n * (1 - ratio)), on the device
    key = torch.where(valid, row_loss, torch.full_like(row_loss, float("inf")))
    order = torch.argsort(key, stable=True)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), device=order.device)
    return rank < k, k


class _SeededGrad:
    """The logits' gradient a criterion's forward wrote at the scale of `seed`: the fp32 device scalar the caller says it WILL hand to
    `loss.backward(seed)` (trainer.TrainStep: its constant ones tensor).  It is handed out once, and only to a backward that receives
    that very tensor, unwritten since the forward; every other backward (another tensor, a seed written to since, a repeated call under
    retain_graph) recomputes at the scale it is given -- from tensors the Function saved with save_for_backward, none of which this
    object holds or clears.  Of the seed only its identity and version are read, so it lives here, outside autograd's version check
    (which would raise where a recomputation is the right answer)."""

    @staticmethod
    def usable(seed, device):
        return seed is not None and seed.dtype == torch.float32 and seed.numel() == 1 and seed.device == device

    def __init__(self, seed=None, pre=None):                 # (no arguments: nothing precomputed, every backward computes)
        self.seed, self.version, self.pre = seed, None if seed is None else seed._version, pre

    def take(self, dloss):
        """the precomputed gradient if `dloss` is the backward it was computed for (None: recompute); it is handed out once"""
        seed = self.seed
        if self.pre is None or dloss.data_ptr() != seed.data_ptr() or dloss.dtype != seed.dtype or seed._version != self.version:
            return None
        return self.spare()

    def spare(self):
        """the precomputed buffer, if it was never handed out, to write a recomputed gradient into (None: allocate)"""
        d, self.pre = self.pre, None
        return d


class CrossEntropyFn(torch.autograd.Function):
    """sum over rows of NLL(log_softmax_fp32(logits), target), ignore_index rows contribute 0
    (engine/criterion/cross_entropy.py:27-67).  logits: [..., V]; a row stride that is no multiple of the vector width is padded here."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, seed=None, stats=None):
        """stats: a StepStats or None.  With it, and on the one-pass path, the kernel's last block also adds the micro-batch's share of
        the step statistics (stats.done is then set: the caller launches nothing more for them).
        seed: see _SeededGrad.  With it the logits' gradient is computed by the forward kernel from the row it already holds (one
        pass over the logits instead of three); a backward that cannot take it runs ce_bwd on the saved logits view."""
        V = logits.shape[-1]
        l2d = _ce_rows(logits)
        t = target.reshape(-1).contiguous()
        ctx.ignore_index, ctx.shape = ignore_index, logits.shape
        ctx.seeded = _SeededGrad()
        if ctx.needs_input_grad[0] and _SeededGrad.usable(seed, l2d.device) and K.cross_entropy_fwd_grad_ok(l2d, V):
            if stats is not None and t.dtype == torch.int64 and t.numel() >= 1:
                lse, row_loss, d, loss = K.cross_entropy_fwd_grad(l2d, t, seed, V, ignore_index, stats.stats, stats.ticket)
                stats.done = True
                ctx.seeded = _SeededGrad(seed, d)
                ctx.save_for_backward(l2d, t, lse)
                return loss
            lse, row_loss, d = K.cross_entropy_fwd_grad(l2d, t, seed, V, ignore_index)
            ctx.seeded = _SeededGrad(seed, d)
        else:
            lse, row_loss = K.cross_entropy_fwd(l2d, t, V, ignore_index)     # (no seed known: the forward does not write a gradient)
        ctx.save_for_backward(l2d, t, lse)
        return K.sum_f32(row_loss)

    @staticmethod
    def backward(ctx, dloss):
        l2d, t, lse = ctx.saved_tensors
        V = l2d.shape[1]
        d = ctx.seeded.take(dloss)
        if d is None:
            gs = dloss.reshape(1).float().contiguous()
            d = K.cross_entropy_bwd(l2d, t, lse, gs, V, ctx.ignore_index, dlogits=ctx.seeded.spare())
        return d[:, :V].view(ctx.shape), None, None, None, None


class StepStats:
    """Where a criterion may add its micro-batch's [sample_size, loss_sum, ntokens] itself: stats fp64[3] and the ticket word of the
    kernel that does it (int32, zero); done: the last forward did."""

    def __init__(self, stats, ticket):
        self.stats, self.ticket, self.done = stats, ticket, False


def cross_entropy_sum(logits, target, ignore_index, seed=None, stats=None):
    if stats is not None:
        stats.done = False
    return CrossEntropyFn.apply(logits, target, ignore_index, seed, stats)


class LabelSmoothedCrossEntropyFn(torch.autograd.Function):
    """label_smoothed_nll_loss fused with the fp32 log-softmax (engine/criterion/label_smoothed_cross_entropy.py:62-191):
    returns (loss_sum, nll_sum, ntokens).  constraint_range = (start, end): only [0,4) U [start,end) of the vocabulary takes
    part (:140-151); constraint_masks: optional bool [rows, V] from the sample; drop_worst_ratio: the worst rows are dropped
    (:83-86) -- selected with a device-side sort, no host sync (the reference's boolean indexing + topk both sync)."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, eps, constraint_range, constraint_masks, drop_worst_ratio):
        V = logits.shape[-1]
        l2d, t, cs, ce, cm, _ = _criterion_rows("label_smoothed_cross_entropy", logits, target, constraint_range, constraint_masks)
        lse, row_loss, row_nll, row_cnt = K.ls_cross_entropy_fwd(l2d, t, V, ignore_index, eps, cs, ce, cm)
        valid = t.ne(ignore_index)
        row_w = None
        if drop_worst_ratio > 0:
            keep, ntok = _drop_rank(row_loss, valid, drop_worst_ratio)
            row_w = keep.float()
            row_loss, row_nll = row_loss * row_w, row_nll * row_w     # (a dropped +inf row: NaN here, 0 in the trie forms' torch.where)
        else:
            ntok = valid.sum()
        ctx.save_for_backward(l2d, t, lse, row_cnt, row_w, cm)
        ctx.cfg = (ignore_index, eps, cs, ce, logits.shape)
        ctx.mark_non_differentiable(ntok)
        return K.sum_f32(row_loss), K.sum_f32(row_nll).detach(), ntok

    @staticmethod
    def backward(ctx, dloss, dnll, dntok):
        l2d, t, lse, row_cnt, row_w, cm = ctx.saved_tensors
        ignore_index, eps, cs, ce, shape = ctx.cfg
        V = l2d.shape[1]
        gs = dloss.reshape(1).float().contiguous()
        d = K.ls_cross_entropy_bwd(l2d, t, lse, row_cnt, row_w, gs, V, ignore_index, eps, cs, ce, cm)
        return d[:, :V].view(shape), None, None, None, None, None, None


def label_smoothed_cross_entropy(logits, target, ignore_index, eps, constraint_range=None, constraint_masks=None,
                                 drop_worst_ratio=0.0):
    return LabelSmoothedCrossEntropyFn.apply(logits, target, ignore_index, eps, constraint_range, constraint_masks,
                                             drop_worst_ratio)


class TrieLabelSmoothedCrossEntropyFn(torch.autograd.Function):
    """LabelSmoothedCrossEntropyFn for closed-set targets, the [rows, V] constraint mask replaced by one trie node per row: row r's
    allowed set is the children of nodes[r] in `trie` (the dict of device arrays of traverse.TraversePlan.to_device: node_edge_off,
    edge_token, N, E), a node of -1 allowing nothing.  Returns (loss_sum, nll_sum, ntokens).  A live target that is not an allowed
    child of its node gives loss = +inf, as the reference's masked log-probability does, and no gradient.
    seed: see _SeededGrad.  With it and without drop_worst the forward launch also writes the logits' gradient
    (kernels.trie_ls_cross_entropy_fwd); every other backward runs kernels.trie_ls_cross_entropy_bwd on the saved rows."""

    @staticmethod
    def forward(ctx, logits, target, nodes, trie, ignore_index, eps, constraint_range, drop_worst_ratio, seed):
        V = logits.shape[-1]
        l2d, t, cs, ce, _, nd = _criterion_rows("trie_label_smoothed_cross_entropy", logits, target, constraint_range, nodes=nodes)
        seeded = drop_worst_ratio <= 0 and ctx.needs_input_grad[0] and _SeededGrad.usable(seed, l2d.device)
        lse, row_loss, row_nll, row_cnt, d = K.trie_ls_cross_entropy_fwd(l2d, t, nd, trie, V, ignore_index, eps, cs, ce,
                                                                         grad_scale=seed if seeded else None, want_grad=seeded)
        ctx.seeded = _SeededGrad(seed, d) if seeded else _SeededGrad()
        valid = t.ne(ignore_index)
        row_w = None
        if drop_worst_ratio > 0:
            row_w, row_loss, row_nll, ntok = _drop_worst(row_loss, row_nll, valid, drop_worst_ratio)
        else:
            ntok = valid.sum()
        ctx.save_for_backward(l2d, t, nd, lse, row_cnt, row_w, trie["node_edge_off"], trie["edge_token"])
        ctx.cfg = (ignore_index, eps, cs, ce, logits.shape, int(trie["N"]), int(trie["E"]))
        ctx.mark_non_differentiable(ntok)
        return K.sum_f32(row_loss), K.sum_f32(row_nll).detach(), ntok

    @staticmethod
    def backward(ctx, dloss, dnll, dntok):
        l2d, t, nd, lse, row_cnt, row_w, off, tok = ctx.saved_tensors
        ignore_index, eps, cs, ce, shape, N, E = ctx.cfg
        V = l2d.shape[1]
        d = ctx.seeded.take(dloss)
        if d is None:
            gs = dloss.reshape(1).float().contiguous()
            trie = {"node_edge_off": off, "edge_token": tok, "N": N, "E": E}
            d = K.trie_ls_cross_entropy_bwd(l2d, t, nd, trie, lse, row_cnt, row_w, gs, V, ignore_index, eps, cs, ce,
                                            dlogits=ctx.seeded.spare())
        return d[:, :V].view(shape), None, None, None, None, None, None, None, None


def trie_label_smoothed_cross_entropy(logits, target, nodes, trie, ignore_index, eps, constraint_range=None, drop_worst_ratio=0.0,
                                      seed=None):
    """-> (loss_sum, nll_sum, ntokens).  nodes: int32, one trie node per row of the [rows, V] view of `logits` (-1: no closed set at
    that position); trie: the device arrays of the answer trie (Task.constraint_trie_on).  seed: as in `cross_entropy_sum`."""
    return TrieLabelSmoothedCrossEntropyFn.apply(logits, target, nodes, trie, ignore_index, eps, constraint_range, drop_worst_ratio,
                                                 seed)


def _drop_worst(row_loss, row_nll, valid, drop_worst_ratio):
    """Drop-worst of the trie forms: the rows _drop_rank drops are set to 0 -> (row_w, row_loss, row_nll, ntokens)."""
    keep, k = _drop_rank(row_loss, valid, drop_worst_ratio)
    row_w = keep.float()
    zero = torch.zeros_like(row_loss)
    return row_w, torch.where(keep, row_loss, zero), torch.where(keep, row_nll, zero), k   # (a dropped +inf row: 0, not NaN)


def _head_inputs(who, feats, weight, bias, target, nodes):
    D = feats.shape[-1]
    f2d = feats.reshape(-1, D)
    if f2d.stride(1) != 1 or f2d.stride(0) % (4 if f2d.dtype == torch.float32 else 8) != 0 or f2d.data_ptr() % 16 != 0:
        f2d = f2d.contiguous()
    if f2d.dtype != weight.dtype:
        raise ValueError(f"{who}: features are {f2d.dtype}, the projection is {weight.dtype}")
    t = target.reshape(-1).contiguous()
    nd = nodes.reshape(-1).to(device=f2d.device, dtype=torch.int32).contiguous()
    if nd.numel() != f2d.shape[0] or t.numel() != f2d.shape[0]:
        raise ValueError(f"{who}: {nd.numel()} nodes and {t.numel()} targets for {f2d.shape[0]} feature rows")
    return f2d, t, nd


class TrieHeadCrossEntropyFn(torch.autograd.Function):
    """TrieLabelSmoothedCrossEntropyFn without the vocabulary projection (csrc/trie_head.hip): the decoder's FEATURES [..., D] go in,
    the logits of each row's node's children, the loss and the compact gradient g [rows, max_degree] come out of one launch, and the
    backward runs the two gradient kernels on g -- dfeats (every row written) and the projection's rows of the batch's tokens.  The
    weight gradient is a PARTIAL writer of `weight._ofa_grad` (kernels._accum(full=False)), so on a tied embedding it composes with the
    dense head of another micro-batch and the embedding's own rows in either order; without a sink it is a zero [V, D] tensor with
    the rows added.  Loss scaling and drop-worst enter in the backward: there is no seeded form."""

    @staticmethod
    def forward(ctx, feats, weight, bias, target, nodes, trie, ignore_index, eps, constraint_range, drop_worst_ratio):
        f2d, t, nd = _head_inputs("trie_head_cross_entropy", feats, weight, bias, target, nodes)
        cs, ce = _range(constraint_range)
        out = K.trie_head_fwd(f2d, weight, bias, t, nd, trie, ignore_index, eps, cs, ce, want_grad=True)
        row_loss, row_nll = out["row_loss"], out["row_nll"]
        valid = t.ne(ignore_index)
        row_w = None
        if drop_worst_ratio > 0:
            row_w, row_loss, row_nll, ntok = _drop_worst(row_loss, row_nll, valid, drop_worst_ratio)
        else:
            ntok = valid.sum()
        ctx.buckets = K.trie_head_buckets(nd, trie) if ctx.needs_input_grad[1] else None      # (this step's rows by node, for dW)
        ctx.save_for_backward(f2d, weight, t, nd, out["g"], row_w)
        ctx.bias_ref, ctx.trie = bias, trie
        ctx.cfg = (ignore_index, cs, ce, feats.shape)
        ctx.mark_non_differentiable(ntok)
        return K.sum_f32(row_loss), K.sum_f32(row_nll).detach(), ntok

    @staticmethod
    def backward(ctx, dloss, dnll, dntok):
        f2d, weight, t, nd, g, row_w = ctx.saved_tensors
        ignore_index, cs, ce, shape = ctx.cfg
        trie, bias = ctx.trie, ctx.bias_ref
        gs = dloss.reshape(1).float().contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = K.trie_head_bwd_dx(g, weight, t, nd, trie, row_w, gs, ignore_index, cs, ce).view(shape)
        if ctx.needs_input_grad[1]:
            gw = _sink(weight)
            gb = _sink(bias) if bias is not None and ctx.needs_input_grad[2] else None
            want_b = bias is not None and ctx.needs_input_grad[2]
            if gw is None:
                dw = torch.zeros_like(weight, memory_format=torch.contiguous_format)
            if want_b and gb is None:
                db = torch.zeros_like(bias)
            K.trie_head_bwd_dw(g, f2d, trie, ctx.buckets, row_w, gs, gw if gw is not None else dw,
                               (gb if gb is not None else db) if want_b else None, cs, ce)
            if gw is not None:
                _sink_done(weight)
            if gb is not None:
                _sink_done(bias)
        return dx, dw, db, None, None, None, None, None, None, None


def trie_head_cross_entropy(feats, weight, bias, target, nodes, trie, ignore_index, eps, constraint_range=None, drop_worst_ratio=0.0):
    """-> (loss_sum, nll_sum, ntokens): trie_label_smoothed_cross_entropy(linear(feats, weight, bias), ...) computed over the children
    of each row's trie node alone -- no [rows, V] logits, no dense dX / dW products.  feats [..., D] (the decoder with
    features_only=True), weight [V, D] / bias [V] or None: the output projection (a tied embedding included); nodes: int32, one trie
    node per feature row (-1: no closed set at that position); trie: Task.constraint_trie_on(device) / TraversePlan.head_arrays."""
    for k in K.HEAD_TRIE_KEYS + ("N", "E", "U", "max_degree"):
        if trie.get(k) is None:
            raise ValueError(f"trie_head_cross_entropy: the trie's device arrays carry no {k!r} (Task.constraint_trie_on / "
                             f"TraversePlan.head_arrays hand out all of them)")
    if not 0 <= drop_worst_ratio < 1:
        raise ValueError(f"trie_head_cross_entropy: drop_worst_ratio must be in [0, 1), got {drop_worst_ratio}")
    return TrieHeadCrossEntropyFn.apply(feats, weight, bias, target, nodes, trie, ignore_index, eps, constraint_range, drop_worst_ratio)


def trie_head_eval(feats, weight, bias, target, nodes, trie, pad, eps, constraint_range=None, acc=None):
    """criterion_eval(nodes=...) from features (validation with the trie-edge head): the forward launch of trie_head_cross_entropy
    with its arg-max output, then eval_stats_add.  Returns (acc, row_loss, row_nll, row_hit); nothing is synchronised."""
    for k in ("node_edge_off", "edge_token", "N", "E", "max_degree"):
        if trie.get(k) is None:
            raise ValueError(f"trie_head_eval: the trie's device arrays carry no {k!r}")
    with torch.no_grad():
        f2d, t, nd = _head_inputs("trie_head_eval", feats.detach(), weight, bias, target, nodes)
        cs, ce = _range(constraint_range)
        out = K.trie_head_fwd(f2d, weight.detach(), None if bias is None else bias.detach(), t, nd, trie, pad, eps, cs, ce,
                              want_grad=False, want_hit=True)
        if acc is None:
            acc = torch.zeros(4, dtype=torch.float64, device=f2d.device)
        K.eval_stats_add(acc, out["row_loss"], out["row_nll"], out["row_hit"], t, pad)
    return acc, out["row_loss"], out["row_nll"], out["row_hit"]


class CtcLayout:
    """Where the sentences of a CTC batch lie in the logits' rows: sentence b is the rows seg[b, 0] + t * row_stride, t < seg[b, 1]
    <= tmax (seg: int32 device tensor [B, >= 2]).  Lengths are device data; tmax is a launch bound taken from shapes."""

    def __init__(self, seg, row_stride, tmax, batch_major=False):
        self.seg, self.row_stride, self.tmax, self.batch_major = seg, int(row_stride), int(tmax), bool(batch_major)

    @classmethod
    def padded(cls, lengths, T, batch_major=False):
        """The T x B x C encoder output: sentence b is rows b, b + B, ...; lengths: device integer tensor [B] (non-pad positions).
        batch_major: the logits are a [T, B, C] VIEW of [B, T, C] storage (what the layer stack hands out); the rows are then read
        in storage order -- sentence b is rows b T, b T + 1, ... -- and no transposed copy is made."""
        B = lengths.numel()
        first = torch.arange(B, dtype=torch.int32, device=lengths.device)
        seg = torch.stack([first * T if batch_major else first, lengths.reshape(-1).to(torch.int32)], 1)
        return cls(seg.contiguous(), 1 if batch_major else B, T, batch_major)

    @classmethod
    def packed(cls, segments):
        """Packed rows: a packing.Segments table on the logits' device (PackPlan.enc_self: q_off, q_len), a sentence's rows contiguous."""
        return cls(segments.table, 1, segments.max_q)


def _ctc_inputs(who, logits, layout, encoder_target):
    """-> (logits as [rows, C] in the row order the layout describes, restore: a [rows, C] gradient -> the logits' shape and layout,
    encoder_target as a contiguous int64 tensor on the logits' device)."""
    C = logits.shape[-1]
    t = encoder_target
    if t.dim() != 2 or t.shape[0] != layout.seg.shape[0]:
        raise ValueError(f"{who}: encoder_target must be [B={layout.seg.shape[0]}, Lmax], got {tuple(t.shape)}")
    t = t.to(device=logits.device, dtype=torch.int64).contiguous()
    shape = logits.shape
    if layout.batch_major:
        if logits.dim() != 3 or not logits.transpose(0, 1).is_contiguous():
            raise ValueError(f"{who}: a batch-major layout needs logits that are a [T, B, C] view of contiguous [B, T, C] storage")
        return logits.transpose(0, 1).reshape(-1, C), lambda d: d.view(shape[1], shape[0], C).transpose(0, 1), t
    l2d = logits.reshape(-1, C) if logits.is_contiguous() else logits.contiguous().view(-1, C)
    return l2d, lambda d: d.view(shape), t


class CtcLossFn(torch.autograd.Function):
    """F.ctc_loss(log_softmax_fp32(logits), labels, blank=0, reduction="sum", zero_infinity) over the sentences of a CtcLayout
    (csrc/ctc.hip; engine/criterion/speech_to_text_loss.py:326-362) -> (loss_sum, per-sentence nll).  The labels are encoder_target -
    ds at the positions that are neither pad nor eos, derived by the kernel.  With a usable seed (see _SeededGrad) the forward's
    launch sequence ends with the gradient launch and the backward hands its result out; otherwise the backward runs that launch
    on the saved alpha / beta slabs at the scale it is given.  A gradient on the per-sentence nll is not supported."""

    @staticmethod
    def forward(ctx, logits, layout, encoder_target, ds, pad, eos, zero_infinity, seed=None, stat=None):
        l2d, ctx.restore, t = _ctc_inputs("ctc_loss", logits, layout, encoder_target)
        lse, _ = K.ctc_rows(l2d)
        st = K.ctc_alpha_beta(l2d, lse, layout.seg, layout.row_stride, layout.tmax, t, ds, pad, eos, zero_infinity)
        ctx.layout, ctx.zero_infinity = layout, bool(zero_infinity)
        ctx.seeded = _SeededGrad()
        if ctx.needs_input_grad[0]:
            if _SeededGrad.usable(seed, l2d.device):
                d = K.ctc_grad(l2d, lse, layout.seg, layout.row_stride, layout.tmax, st, seed, zero_infinity)
                ctx.seeded = _SeededGrad(seed, d)
            ctx.save_for_backward(l2d, lse, st["alpha"], st["beta"], st["meta"], st["L"], st["nll_raw"])
            ctx.Lmax = st["Lmax"]
        nll = st["nll"]
        ctx.mark_non_differentiable(nll)
        # (the sentences' fp64 values are summed and the sum rounded once: an fp32 sum would round at the size of the loss per addend)
        total = st["nll64"].sum()
        if stat is not None:
            stat += total
        return total.float(), nll

    @staticmethod
    def backward(ctx, dloss, dnll):
        l2d, lse, alpha, beta, meta, L, nll_raw = ctx.saved_tensors
        d = ctx.seeded.take(dloss)
        if d is None:
            lay = ctx.layout
            st = dict(alpha=alpha, beta=beta, meta=meta, L=L, nll_raw=nll_raw, Lmax=ctx.Lmax)
            d = K.ctc_grad(l2d, lse, lay.seg, lay.row_stride, lay.tmax, st, dloss.reshape(1).float().contiguous(), ctx.zero_infinity,
                           out=ctx.seeded.spare())
        return ctx.restore(d), None, None, None, None, None, None, None, None


def ctc_loss(logits, layout, encoder_target, ds, pad, eos, zero_infinity, seed=None, stat=None):
    """-> (loss_sum fp32 scalar, per_sentence_nll fp32 [B]).  stat: an fp64 device accumulator [1] the summed loss is added to BEFORE its
    rounding to fp32 (the step's and the validation pass's ctc_loss statistics), on the device, nothing synchronised.  logits [..., C] in fp32 / bf16 / fp16 (the padded T x B x C encoder
    projection, or packed rows), layout: a CtcLayout, encoder_target [B, Lmax] integer.  Blank is class 0 (the `ds` row itself).
    Infeasible sentences (target longer than the input, repeats without room for the blank, a label outside [1, C)): nll 0 and a zero
    gradient with zero_infinity, +inf and NaN gradient rows without.  Refuses C and Lmax above kernels.ctc_limits() with a ValueError."""
    return CtcLossFn.apply(logits, layout, encoder_target, int(ds), int(pad), int(eos), bool(zero_infinity), seed, stat)


def ctc_greedy_decode(logits, layout):
    """Greedy CTC decode on the device: per sentence the row arg-max (ties: the lowest class), consecutive duplicates collapsed, blanks
    (class 0) dropped.  -> (tokens int32 [B, tmax], -1 behind each sentence's tokens; lengths int32 [B]); nothing is synchronised."""
    with torch.no_grad():
        if layout.batch_major:
            l2d = logits.detach().transpose(0, 1).reshape(-1, logits.shape[-1])
        else:
            l2d = logits.detach().reshape(-1, logits.shape[-1])
        _, am = K.ctc_rows(l2d, want_argmax=True)
        return K.ctc_greedy_decode(am, layout.seg, layout.row_stride, layout.tmax)


def edit_distance(a, b):
    """Levenshtein distance of two sequences, on the host in plain Python: the unit-level error count of a greedy CTC decode against
    its labels (speech_to_text_loss.py:294-300 uses the `editdistance` package for it).  Word-level WER, post_process and the KenLM
    decoder are out of scope."""
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


class EncoderCtcLogitsFn(torch.autograd.Function):
    """enc . weight[ds:de]^T (speech_to_text_loss.py:217-225).  The weight gradient belongs to rows ds:de of the (tied) embedding: with a
    gradient sink it is accumulated into that row range of the arena view through kernels._accum, like every other writer of the
    parameter in the step; without one it is a zero [V, D] tensor with the rows stored."""

    @staticmethod
    def forward(ctx, x2d, weight, ds, de):
        ctx.save_for_backward(x2d, weight)
        ctx.range = (ds, de)
        return K.gemm(x2d, weight[ds:de], False, True)

    @staticmethod
    def backward(ctx, dy):
        x2d, weight = ctx.saved_tensors
        ds, de = ctx.range
        dy = dy if dy.stride(-1) == 1 else dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = K.gemm(dy, weight[ds:de], False, False)
        if ctx.needs_input_grad[1]:
            gw = _sink(weight)
            if gw is not None:
                K.gemm(dy, x2d, True, False, out=gw[ds:de], accumulate=True)
                _sink_done(weight)
            else:
                dw = torch.zeros_like(weight, memory_format=torch.contiguous_format)
                K.gemm(dy, x2d, True, False, out=dw[ds:de])
        return dx, dw, None, None


def encoder_ctc_logits(enc, weight, ds, de):
    """The CTC logits [..., de - ds] of the encoder output enc [..., D]: its projection onto rows ds:de of the token embedding."""
    ds, de = int(ds), int(de)
    if not 0 <= ds < de <= weight.shape[0]:
        raise ValueError(f"encoder_ctc_logits: rows [{ds}, {de}) of a [{weight.shape[0]}, {weight.shape[1]}] embedding")
    x2d, restore = rows_view(enc)
    return restore(EncoderCtcLogitsFn.apply(x2d, weight, ds, de))


class ScstLossFn(torch.autograd.Function):
    """Self-critical sequence training loss (engine/criterion/scst_loss.py:24-36, 214-233): sum over rows of
    reward[sentence] * NLL(log_softmax_fp32(logits over the allowed vocabulary), target), ignore_index rows contributing 0; returns
    (loss_sum, ntokens).  The kernel writes the logits' gradient in the pass that computes the loss (kernels.scst_loss_fwd_grad)."""

    @staticmethod
    def forward(ctx, logits, target, reward, ignore_index, constraint_range, row_seq, seed):
        V = logits.shape[-1]
        l2d, t, cs, ce, _, _ = _criterion_rows("scst_loss", logits, target, constraint_range)
        w = reward.reshape(-1).to(device=l2d.device, dtype=torch.float32).contiguous()
        rows = l2d.shape[0]
        if row_seq is not None:
            row_seq = row_seq.reshape(-1).to(device=l2d.device, dtype=torch.int32).contiguous()
            if row_seq.numel() != rows:
                raise ValueError(f"scst_loss: row_seq has {row_seq.numel()} entries for {rows} rows")
            rps = 1
        else:
            if w.numel() == 0 or rows % w.numel() != 0:
                raise ValueError(f"scst_loss: {rows} rows do not divide into {w.numel()} sentences (pass row_seq)")
            rps = rows // w.numel()
        seeded = ctx.needs_input_grad[0] and _SeededGrad.usable(seed, l2d.device)
        lse, row_loss, d = K.scst_loss_fwd_grad(l2d, t, w, seed if seeded else None, V, ignore_index, rps, row_seq, cs, ce)
        ctx.seeded = _SeededGrad(seed, d) if seeded else _SeededGrad()      # (a backward that cannot take it runs the same entry again)
        ctx.save_for_backward(l2d, t, w, row_seq)
        ctx.cfg = (ignore_index, rps, cs, ce, logits.shape)
        ntok = t.ne(ignore_index).sum()
        ctx.mark_non_differentiable(ntok)
        return K.sum_f32(row_loss), ntok

    @staticmethod
    def backward(ctx, dloss, dntok):
        l2d, t, w, row_seq = ctx.saved_tensors
        ignore_index, rps, cs, ce, shape = ctx.cfg
        V = l2d.shape[1]
        d = ctx.seeded.take(dloss)
        if d is None:
            gs = dloss.reshape(1).float().contiguous()
            _, _, d = K.scst_loss_fwd_grad(l2d, t, w, gs, V, ignore_index, rps, row_seq, cs, ce)
        return d[:, :V].view(shape), None, None, None, None, None, None


def scst_loss(logits, target, reward, ignore_index, constraint_range=None, row_seq=None, seed=None):
    """-> (loss_sum, ntokens).  reward: one value per sentence; row r of the [rows, V] view of `logits` belongs to sentence row_seq[r],
    or to r // (rows / sentences) without a map (logits [sentences, Tt, V]).  seed: as in `cross_entropy_sum`."""
    return ScstLossFn.apply(logits, target, reward, ignore_index, constraint_range, row_seq, seed)


def criterion_eval(logits, target, pad, eps, constraint_range=None, constraint_masks=None, nodes=None, trie=None, acc=None):
    """Validation's criterion (engine/criterion/label_smoothed_cross_entropy.py:114-198 in eval mode), no autograd: one read of the
    [..., V] logits gives per row the label-smoothed loss, the NLL and "the target is the arg-max of the allowed logits"
    (kernels.criterion_eval), and a second, single-block launch adds [ntokens, loss_sum, nll_sum, n_correct] to `acc` (fp64 [4];
    None: a fresh zero accumulator) in a fixed order.  The allowed set as in label_smoothed_cross_entropy (range, byte masks) or
    trie_label_smoothed_cross_entropy (nodes + trie).  Returns (acc, row_loss, row_nll, row_hit); nothing is synchronised."""
    V = logits.shape[-1]
    if nodes is not None and constraint_masks is not None:
        raise ValueError("criterion_eval: a closed set comes as constraint_masks or as nodes, not both")
    with torch.no_grad():
        l2d, t, cs, ce, cm, nd = _criterion_rows("criterion_eval", logits.detach(), target, constraint_range, constraint_masks, nodes)
        row_loss, row_nll, row_hit = K.criterion_eval(l2d, t, V, pad, eps, cs, ce, cm, nd, trie)
        if acc is None:
            acc = torch.zeros(4, dtype=torch.float64, device=l2d.device)
        K.eval_stats_add(acc, row_loss, row_nll, row_hit, t, pad)
    return acc, row_loss, row_nll, row_hit


def _rows_padded(logits):
    """[..., V] tensor -> ([rows, V] view with last dim contiguous, ld)."""
    V = logits.shape[-1]
    try:
        l2d = logits.view(-1, V)
    except RuntimeError:
        l2d = logits.reshape(-1, V)
    if l2d.stride(1) != 1:
        l2d = l2d.contiguous()
    return l2d, l2d.stride(0)


class ProbsFn(torch.autograd.Function):
    """fp32 softmax / log-softmax over the last dim (get_normalized_probs, model/ofa.py:287-299)."""

    @staticmethod
    def forward(ctx, logits, log_probs):
        l2d, ld = _rows_padded(logits)
        rows, V = l2d.shape
        y = K.probs_fwd(l2d, V, ld, log_probs)
        ctx.save_for_backward(y)
        ctx.meta = (logits.shape, logits.dtype, log_probs)
        return y.view(*logits.shape)

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        shape, dtype, log_probs = ctx.meta
        V = shape[-1]
        d = K.probs_bwd(dy.reshape(-1, V).float().contiguous(), y, V, dtype, log_probs)
        return d[:, :V].view(shape), None


def log_softmax_fp32(logits):
    return ProbsFn.apply(logits, True)


def softmax_fp32(logits):
    return ProbsFn.apply(logits, False)


# ---------------------------------------------------------------------------------------------- convolution stack
# Feature maps travel as (rows [B*H*W, C], (B, H, W)) pairs: NHWC rows, so 1x1 convolutions are plain GEMMs.
class Conv2dFn(torch.autograd.Function):
    """nn.Conv2d(bias optional) on NHWC rows (or on the [B,C,H,W] image itself when `nchw`): im2col + MFMA GEMM
    (module/resnet.py:22-38, module/subsample.py:29-35).  weight keeps torch's [Cout, Cin, kh, kw] layout (state dict)."""

    @staticmethod
    def forward(ctx, x, weight, bias, geom, mailbox=None, want_stats=False):
        """-> (y, stats): stats = the column statistics of y as partial rows [groups, 2, Cout] fp64 left by the GEMM's epilogue when
        `want_stats` (a BatchNorm follows: conv_bn) and the selected kernel can produce them, else an empty tensor."""
        B, H, W, stride, pad, nchw = geom
        ctx.mailbox = mailbox
        Cout, Cin, kh, kw = weight.shape
        direct = kh == 1 and kw == 1 and stride == 1 and pad == 0 and not nchw
        if direct:
            col, Ho, Wo = x, H, W
            w2 = weight.view(Cout, Cin)
        else:
            col, Ho, Wo = K.im2col(x, B, H, W, Cin, kh, kw, stride, pad, nchw)
            # taps (kh, kw, c), like the columns: a view when the weight already lives in that order (trainer.FlatParams keeps
            # spatial convolution weights channels_last in its arena), a permuted copy otherwise
            w2 = weight.permute(0, 2, 3, 1).reshape(Cout, kh * kw * Cin)
            if col.shape[1] != w2.shape[1]:
                w2 = torch.nn.functional.pad(w2, (0, col.shape[1] - w2.shape[1]))
            w2 = w2.contiguous()
        stats = None
        if want_stats:
            y, stats = K.gemm_colstat(col, w2, bias=bias)
        else:
            y = K.gemm(col, w2, False, True, bias=bias)
        if stats is None:
            stats = torch.empty(0, dtype=torch.float64, device=y.device)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)         # (no zero-filled fp64 "gradient" of the statistics output: it was one fill launch per layer)
        ctx.save_for_backward(col, w2)
        ctx.geom = (B, H, W, Cin, kh, kw, stride, pad, nchw, direct)
        ctx.refs = (weight, bias)
        return y, stats

    @staticmethod
    def backward(ctx, dy, _dstats=None):
        if dy is None:
            return None, None, None, None, None, None
        col, w2 = ctx.saved_tensors
        B, H, W, Cin, kh, kw, stride, pad, nchw, direct = ctx.geom
        weight, bias = ctx.refs
        Cout = weight.shape[0]
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0] and not nchw:
            skip = ctx.mailbox.pop() if ctx.mailbox else None          # the residual branch's gradient of the same input (ResidualMailbox)
            if skip is not None and direct and skip.shape == col.shape and skip.dtype == dy.dtype and skip.is_contiguous():
                dx = K.gemm(dy, w2, False, False, out=skip, accumulate=True)      # dX = dY W + dres: the add rides in the GEMM epilogue
            else:
                dcol = K.gemm(dy, w2, False, False)
                dx = dcol if direct else K.col2im(dcol, B, H, W, Cin, kh, kw, stride, pad)
                if skip is not None:
                    dx = dx + skip
        gw = _sink(weight)
        if gw is not None and not direct:                                         # spatial taps: only when the arena holds them in
            g2 = gw.permute(0, 2, 3, 1)                                           # the GEMM's (kh, kw, c) order, unpadded
            gw = g2 if (g2.is_contiguous() and col.shape[1] == kh * kw * Cin) else None
        if gw is not None:                                                        # dW += dY^T X straight into the arena,
            _wgrad(dy, col, gw.view(Cout, kh * kw * Cin), 1.0, weight)            # queued for a grouped launch (flush_wgrads)
            dw = None
        else:
            dw2 = K.gemm(dy, col, True, False)                                    # [Cout, Kpad]
            if direct:
                dw = dw2.view(weight.shape)
            else:
                dw = dw2[:, :kh * kw * Cin].reshape(Cout, kh, kw, Cin).permute(0, 3, 1, 2)
        db = K.colsum(dy, out_dtype=weight.dtype) if bias is not None else None
        return dx, dw, db, None, None, None


def conv2d(x, weight, bias, B, H, W, stride=1, pad=0, nchw=False, grad_mailbox=None):
    """-> (rows [B*Ho*Wo, Cout], Ho, Wo).  grad_mailbox: see batch_norm."""
    kh, kw = weight.shape[2], weight.shape[3]
    y, _ = Conv2dFn.apply(x, weight, bias, (B, H, W, stride, pad, nchw), grad_mailbox, False)
    return y, K.conv_out_size(H, kh, stride, pad), K.conv_out_size(W, kw, stride, pad)


class _ConvBn:
    epilogue_stats = True    # (tests / A-B tools may clear it: every BatchNorm then runs its own statistics pass)


def conv_bn(x, conv, bn, B, H, W, relu=False, residual=None, nchw=False, conv_mailbox=None, bn_mailbox=None):
    """BatchNorm(conv(x)) [+ residual] [ReLU] -- every convolution of the ResNet trunk is followed by a BatchNorm (module/resnet.py:
    105-128, 232-246).  In training the statistics pass over the convolution's output does not exist: the GEMM's epilogue leaves the
    per-channel (sum, sum of squares) of the rounded tile it holds as partial rows (ofa_gemm_colstat) and the BatchNorm finalises
    from those.  Falls back to the separate statistics kernel when the GEMM plan cannot produce them (split-K, fp32), for
    SyncBatchNorm layers and in eval mode.  -> (rows, Ho, Wo)."""
    weight = conv.weight
    kh, kw = weight.shape[2], weight.shape[3]
    stride, pad = conv.stride[0], conv.padding[0]
    training = bn.training or bn.running_mean is None
    want = (_ConvBn.epilogue_stats and training and x.is_cuda and weight.dtype in (torch.bfloat16, torch.float16)
            and _bn_sync_group(bn) is None)
    y, stats = Conv2dFn.apply(x, weight, conv.bias, (B, H, W, stride, pad, nchw), conv_mailbox, want)
    out = batch_norm(y, bn, relu=relu, residual=residual, grad_mailbox=bn_mailbox, stats=stats if stats.numel() else None)
    return out, K.conv_out_size(H, kh, stride, pad), K.conv_out_size(W, kw, stride, pad)


class _BnScope:
    pending = None


class bn_scope:
    """`with ops.bn_scope():` around a backbone's forward: the `num_batches_tracked += 1` of every BatchNorm inside becomes ONE
    batched launch at exit instead of one 4 us launch per layer (94 per step in a ResNet-101 backbone)."""

    def __enter__(self):
        self.outer = _BnScope.pending
        _BnScope.pending = []
        return self

    def __exit__(self, *exc):
        counters, _BnScope.pending = _BnScope.pending, self.outer
        if counters and exc[0] is None:
            torch._foreach_add_(counters, 1)
        return False


class BatchNormFn(torch.autograd.Function):
    """nn.BatchNorm2d (+ optional residual add and ReLU fused, module/resnet.py:105-128) on NHWC rows."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean, running_var, training, momentum, eps, relu, mailbox=None, stats=None):
        if stats is not None and training:       # the producing convolution's GEMM left the column statistics (conv_bn)
            y, mean, rstd = K.batchnorm_fwd_apply(x, weight, bias, running_mean, running_var, stats, momentum, eps, relu, residual,
                                                  groups=stats.shape[0])
        else:
            y, mean, rstd = K.batchnorm_fwd(x, weight, bias, running_mean, running_var, training, momentum, eps, relu, residual)
        ctx.save_for_backward(x, y, weight, mean, rstd)
        ctx.mailbox = mailbox
        ctx.cfg = (training, relu, residual is not None)
        ctx.bias_ref = bias
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, mean, rstd = ctx.saved_tensors
        training, relu, has_res = ctx.cfg
        gw, gb = _sink(weight), _sink(ctx.bias_ref)
        if gw is not None and gb is not None and weight.requires_grad:
            dx, dres, _, _ = K.batchnorm_bwd(dy, y, x, weight, mean, rstd, training, relu, has_res, dgamma=gw, dbeta=gb,
                                             beta=ctx.bias_ref)
            _sink_done(weight)
            _sink_done(ctx.bias_ref)
            dg = db = None
        else:
            dx, dres, dg, db = K.batchnorm_bwd(dy, y, x, weight, mean, rstd, training, relu, has_res, beta=ctx.bias_ref)
        if ctx.mailbox is not None and dres is not None:
            ctx.mailbox.append(dres)             # handed to the consumer named at forward time, which adds it inside its own kernel
            dres = None
        return dx, dres, dg, db, None, None, None, None, None, None, None, None


def _bn_all_reduce(t, group):
    """SUM of a statistics tensor over the data-parallel ranks (the one exchange of a SyncBatchNorm layer, each way)."""
    import torch.distributed as dist
    if t.is_cuda and torch.cuda.is_current_stream_capturing() and dist.get_backend(group) != "nccl":
        raise NotImplementedError("sync_bn inside a captured step needs the nccl (RCCL) backend: host-side collectives cannot be captured")
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


class SyncBatchNormFn(torch.autograd.Function):
    """nn.SyncBatchNorm (module/layer.py:26-27, adaptor/image_resnet.py:87-90 `sync_bn`) on NHWC rows, training mode: the batch
    statistics cover every rank's rows.  Same kernels as BatchNormFn, cut in two phases each way around ONE all-reduce of the
    per-channel sums ([2C + 1] fp64 forward -- the row count rides along, so ranks may hold different batch sizes and nobody
    syncs --, [2, C] fp32 backward); the parameter gradients stay rank-local sums, which the gradient exchange adds up like every
    other gradient (torch's own SyncBatchNorm backward does the same)."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean, running_var, momentum, eps, relu, group, mailbox=None):
        sums = _bn_all_reduce(K.batchnorm_fwd_stats(x), group)
        y, mean, rstd = K.batchnorm_fwd_apply(x, weight, bias, running_mean, running_var, sums, momentum, eps, relu, residual)
        ctx.save_for_backward(x, y, weight, mean, rstd, sums)
        ctx.mailbox, ctx.group = mailbox, group
        ctx.cfg = (relu, residual is not None)
        ctx.bias_ref = bias
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, mean, rstd, fsums = ctx.saved_tensors
        relu, has_res = ctx.cfg
        regate = ctx.bias_ref if (relu and not has_res) else None
        gw, gb = _sink(weight), _sink(ctx.bias_ref)
        sink = gw is not None and gb is not None and weight.requires_grad
        sums, dg, db = K.batchnorm_bwd_stats(dy, y, x, weight, mean, rstd, relu, regate, gw if sink else None, gb if sink else None)
        if sink:
            _sink_done(weight)
            _sink_done(ctx.bias_ref)
            dg = db = None
        _bn_all_reduce(sums, ctx.group)
        dx, dres = K.batchnorm_bwd_dx(dy, y, x, weight, mean, rstd, sums, fsums[-1:], relu, has_res, regate)
        if ctx.mailbox is not None and dres is not None:
            ctx.mailbox.append(dres)
            dres = None
        return dx, dres, dg, db, None, None, None, None, None, None, None


_SYNC_BN_GROUP = []      # the SyncBatchNorm layers' own communicator (created collectively, once per process)


def sync_bn_process_group():
    """The default `sync_bn` exchange runs on its OWN communicator, never on the group the gradient buckets use: a communicator
    matches collectives by issue order, and the bucket reducer issues its all-reduces at rank-local points of backward (a rank whose
    step structure is already learned launches buckets from inside backward, a rank that still learns launches all of them at
    finish()), so SyncBatchNorm's backward exchange would land between different buckets on different ranks.  Created on
    first use by a collective `new_group` -- every rank reaches its first SyncBatchNorm layer in the same (eager, warm-up) step -- or
    up front by TrainStep."""
    import torch.distributed as dist
    if not _SYNC_BN_GROUP:
        _SYNC_BN_GROUP.append(dist.new_group())
    return _SYNC_BN_GROUP[0]


def _bn_sync_group(bn):
    """The process group a BatchNorm layer synchronises its training statistics over, or None: `bn._ofa_sync` is set by the owner
    (ImageResnetAdaptor with cfg.sync_bn) to True (all ranks, on the layers' dedicated communicator) or to a group; a single-rank job
    needs no exchange."""
    sync = getattr(bn, "_ofa_sync", None)
    if sync is None or sync is False:
        return None
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return None
    if sync is True:
        return (sync_bn_process_group(),) if dist.get_world_size() > 1 else None
    return (sync,) if dist.get_world_size(sync) > 1 else None


def batch_norm(x, bn: torch.nn.BatchNorm2d, relu=False, residual=None, grad_mailbox=None, stats=None):
    """bn holds torch's parameters / buffers (state-dict parity); statistics follow bn.training like nn.BatchNorm2d.
    grad_mailbox (a list shared with ONE conv2d call on the same tensor `residual`): in backward the residual's gradient is not
    returned to autograd (which would add it to the other consumer's gradient with a separate elementwise kernel) but left in the
    mailbox, and that convolution's input-gradient GEMM accumulates onto it in its epilogue (an identity bottleneck: x feeds conv1
    AND the residual add, module/resnet.py:112-137)."""
    training = bn.training or bn.running_mean is None
    momentum = 0.1 if bn.momentum is None else bn.momentum
    if training and bn.num_batches_tracked is not None:
        if _BnScope.pending is not None:
            _BnScope.pending.append(bn.num_batches_tracked)        # one batched increment when the backbone's forward ends
        else:
            bn.num_batches_tracked.add_(1)
    rm, rv = bn.running_mean, bn.running_var
    cast = rm is not None and rm.dtype != torch.float32       # model.bfloat16() casts the buffers too: keep the update in fp32
    if cast:
        rm, rv = rm.float(), rv.float()
    sync = _bn_sync_group(bn) if training else None
    if sync is not None:
        y = SyncBatchNormFn.apply(x, residual, bn.weight, bn.bias, rm, rv, momentum, bn.eps, relu, sync[0], grad_mailbox)
    else:
        y = BatchNormFn.apply(x, residual, bn.weight, bn.bias, rm, rv, training, momentum, bn.eps, relu, grad_mailbox, stats)
    if cast and training:
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    return y


class MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, geom):
        B, H, W, k, stride, pad = geom
        y, arg, Ho, Wo = K.maxpool_fwd(x, B, H, W, x.shape[1], k, stride, pad)
        ctx.save_for_backward(arg)
        ctx.geom = geom + (x.shape[1],)
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        B, H, W, k, stride, pad, C = ctx.geom
        return K.maxpool_bwd(dy, arg, B, H, W, C, k, stride, pad), None


def max_pool(x, B, H, W, k, stride, pad):
    y = MaxPoolFn.apply(x, (B, H, W, k, stride, pad))
    return y, K.conv_out_size(H, k, stride, pad), K.conv_out_size(W, k, stride, pad)


class ReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = K.relu(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return K.relu(dy, y)


def relu(x):
    x2d, restore = rows_view(x)
    return restore(ReluFn.apply(x2d))


# ---------------------------------------------------------------------------------------------- text-to-speech (csrc/conv1d.hip, tacotron_loss.hip)
class Conv1dFn(torch.autograd.Function):
    """nn.Conv1d(odd k, padding (k-1)/2) over time on batch-major channels-last rows [B*T, Cin]: time-unfold + MFMA GEMM
    (adaptor/audio.py:743-748).  weight keeps torch's [Cout, Cin, k] layout (state dict); the GEMM reads a (k, c)-ordered copy made
    here per call (Cout * k * Cin elements read and written: 0.4 M for the widest postnet layer, against rows * k * Cin of the unfold)."""

    @staticmethod
    def forward(ctx, x, weight, bias, geom, want_stats=False):
        """-> (y [B*T, Cout], stats): as Conv2dFn.forward."""
        B, T = geom
        Cout, Cin, k = weight.shape
        if k % 2 == 0:
            raise OfaError(f"conv1d: kernel size {k} is even (the length-keeping padding (k-1)/2 needs an odd one)")
        if x.dim() != 2 or x.shape[0] != B * T or x.shape[1] != Cin:
            raise OfaError(f"conv1d: rows {tuple(x.shape)} are not [B*T, Cin] = [{B}*{T}, {Cin}]")
        col = K.unfold1d(x, B, T, Cin, k)
        w2 = weight.permute(0, 2, 1).reshape(Cout, k * Cin)
        if col.shape[1] != w2.shape[1]:
            w2 = torch.nn.functional.pad(w2, (0, col.shape[1] - w2.shape[1]))
        w2 = w2.contiguous()
        stats = None
        if want_stats:
            y, stats = K.gemm_colstat(col, w2, bias=bias)
        else:
            y = K.gemm(col, w2, False, True, bias=bias)
        if stats is None:
            stats = torch.empty(0, dtype=torch.float64, device=y.device)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(col, w2)
        ctx.geom = (B, T, Cin, k)
        ctx.has_bias, ctx.wdtype = bias is not None, weight.dtype
        return y, stats

    @staticmethod
    def backward(ctx, dy, _dstats=None):
        if dy is None:
            return None, None, None, None, None
        col, w2 = ctx.saved_tensors
        B, T, Cin, k = ctx.geom
        Cout = w2.shape[0]
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.fold1d(K.gemm(dy, w2, False, False), B, T, Cin, k)
        dw = None
        if ctx.needs_input_grad[1]:
            dw2 = K.gemm(dy, col, True, False)                                    # [Cout, Kpad]
            dw = dw2[:, :k * Cin].reshape(Cout, k, Cin).permute(0, 2, 1)
        db = K.colsum(dy, out_dtype=ctx.wdtype) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, dw, db, None, None


def conv1d_bn(x, conv, bn, B, T):
    """BatchNorm1d(Conv1d(x)) on batch-major channels-last rows [B*T, Cin] -> [B*T, Cout]: a layer of the Tacotron postnet up to its
    tail (adaptor/audio.py:743-749), over the PADDED layout -- the reference convolves and normalises padded frames too.  In training
    the GEMM's epilogue leaves the column statistics (conv_bn); eval mode uses the running statistics."""
    weight = conv.weight
    if conv.stride[0] != 1 or conv.dilation[0] != 1 or conv.groups != 1 or conv.padding[0] != (weight.shape[2] - 1) // 2:
        raise OfaError("conv1d_bn: only stride 1, dilation 1, groups 1 and padding (k-1)/2")
    training = bn.training or bn.running_mean is None
    want = (_ConvBn.epilogue_stats and training and x.is_cuda and weight.dtype in (torch.bfloat16, torch.float16)
            and _bn_sync_group(bn) is None)
    y, stats = Conv1dFn.apply(x, weight, conv.bias, (B, T), want)
    return batch_norm(y, bn, stats=stats if stats.numel() else None)


class TanhDropoutFn(torch.autograd.Function):
    """y = dropout_p(tanh(x)) in one pass; the backward reads dy and y and regenerates the mask (nothing but y is kept)."""

    @staticmethod
    def forward(ctx, x, p):
        seed, off, base = _Rng.reserve(x.numel(), x.device) if p > 0 else (0, 0, None)
        ctx.p, ctx.seed, ctx.off, ctx.base = p, seed, off, base
        y = K.tanh_dropout_fwd(x, p, seed, off, base)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return K.tanh_dropout_bwd(dy, y, ctx.p, ctx.seed, ctx.off, ctx.base), None


def tanh_dropout(x, p, training):
    """dropout(tanh(x)) (the tail of the postnet's inner layers, adaptor/audio.py:751-752); plain tanh when not training / p == 0."""
    x2d, restore = rows_view(x)
    return restore(TanhDropoutFn.apply(x2d, float(p) if training else 0.0))


class Tacotron2LossFn(torch.autograd.Function):
    """engine/criterion/tacotron2_loss.py:169-198 in one launch (csrc/tacotron_loss.hip) -> (loss, terms = [l1, mse, eos]).  With a
    usable seed (see _SeededGrad) the forward's one pass writes the three gradients and the backward hands them out; otherwise the
    backward runs the kernel again at the scale it is given.  A gradient on the terms is not supported."""

    @staticmethod
    def forward(ctx, feat_out, post, eos_out, target, lengths, pos_weight, reduction, seed=None):
        need = any(ctx.needs_input_grad[:3])
        ctx.seeded = _SeededGrad()
        ctx.cfg = (float(pos_weight), reduction, feat_out.shape, post.shape, eos_out.shape)
        pre = need and _SeededGrad.usable(seed, feat_out.device)
        out, d = K.tacotron2_loss(feat_out, post, target, eos_out, lengths, pos_weight, reduction, seed=seed if pre else None, grad=pre)
        if pre:
            ctx.seeded = _SeededGrad(seed, d)
        if need:
            ctx.save_for_backward(feat_out, post, eos_out, target, lengths)
        terms = out[1:4]
        ctx.mark_non_differentiable(terms)
        return out[0], terms

    @staticmethod
    def backward(ctx, dloss, _dterms=None):
        feat_out, post, eos_out, target, lengths = ctx.saved_tensors
        pos_weight, reduction, s_feat, s_post, s_eos = ctx.cfg
        d = ctx.seeded.take(dloss)
        if d is None:
            _, d = K.tacotron2_loss(feat_out, post, target, eos_out, lengths, pos_weight, reduction,
                                    seed=dloss.reshape(1).float().contiguous(), grad=True, grads=ctx.seeded.spare())
        return d[0].view(s_feat), d[1].view(s_post), d[2].view(s_eos), None, None, None, None, None


def tacotron2_loss(feat_out, post, eos_out, target, lengths, bce_pos_weight=1.0, reduction="mean", seed=None):
    """-> (loss fp32 scalar, terms fp32 [3] = (l1_loss, mse_loss, eos_loss)), `compute_loss` of the reference's ofa_tacotron2 criterion:
    feat_out (before the postnet), post (after), target [B, T, F], eos_out [B, T, 1] or [B, T], lengths int64 [B] on the device."""
    if reduction not in K.TACOTRON_REDUCTIONS:
        raise ValueError(f"tacotron2_loss: unknown reduction {reduction!r} (mean | sum)")
    if target.dtype != feat_out.dtype:
        target = target.to(feat_out.dtype)
    return Tacotron2LossFn.apply(feat_out, post, eos_out, target, lengths, float(bce_pos_weight), reduction, seed)


def tacotron2_eval(feat_out, post, eos_out, target, lengths, bce_pos_weight=1.0, reduction="mean"):
    """The validation form: the four scalars (loss, l1, mse, eos) fp32 [4], no gradient and no extra pass."""
    if target.dtype != feat_out.dtype:
        target = target.to(feat_out.dtype)
    return K.tacotron2_loss(feat_out, post, target, eos_out, lengths, bce_pos_weight, reduction)[0]


# ---------------------------------------------------------------------------------------------- motion diffusion training (csrc/diffusion.hip)
def diffusion_q_sample(x0, noise, t, schedule, width, dtype, known_w=None, masks=None):
    """q-sample, the in-betweening mix and the zero padding to `width` columns in one pass (module/diffusion.py:160 `add_noise`,
    adaptor/motion_6d.py:90-97) -> [B, T, width] of `dtype`, the rows the frame encoder's first GEMM reads.  x0, noise fp32 [B, T, Dd];
    t int64 [B]; schedule: a diffusion.NoiseSchedule.  The inputs are data: no backward."""
    tab = schedule.on(x0.device)
    return K.diffusion_q_sample(x0, noise, t, tab.sqrt_acp, tab.sqrt_1m_acp, width, dtype, known_w=known_w, masks=masks)


class FilmFn(torch.autograd.Function):
    """out = (rows[r, :D] + 1) * h + rows[r, D:] (adaptor/motion_6d.py:106-107 on gathered table rows); the backward sums the rows'
    gradient in fp32 in a fixed order (ofa_film_bwd)."""

    @staticmethod
    def forward(ctx, h, rows, row_of):
        ctx.save_for_backward(h, rows, row_of)
        return K.film_fwd(h, rows, row_of)

    @staticmethod
    def backward(ctx, dout):
        h, rows, row_of = ctx.saved_tensors
        dh, drows = K.film_bwd(dout, h, rows, row_of)
        return dh, drows, None


def film(h, rows, row_of=None):
    """The noise-level modulation of h [B, T, D] by rows [R, 2D] = (scale | shift): position (b, t) takes row row_of[b, t] (int32
    [B, T]; R = B + 1 and every entry its sentence b or the shared row B) or, without row_of, row b."""
    return FilmFn.apply(h, rows, row_of)


class DiffusionLossFn(torch.autograd.Function):
    """module/diffusion.py:156-173 `p_losses` and the criterion's reduction (engine/criterion/diffusion_loss.py:50-57) in one launch.
    With a usable seed (see _SeededGrad) the forward's one pass writes the prediction's gradient and the backward hands it out;
    otherwise the backward runs the kernel again at the scale it is given."""

    @staticmethod
    def forward(ctx, pred, target, t, masks, w, scale, seed=None):
        need = ctx.needs_input_grad[0]
        ctx.seeded = _SeededGrad()
        ctx.scale = float(scale)
        pre = need and _SeededGrad.usable(seed, pred.device)
        out, d = K.diffusion_loss(pred, target, t, w, scale, masks=masks, seed=seed if pre else None, grad=pre)
        if pre:
            ctx.seeded = _SeededGrad(seed, d)
        if need:
            ctx.save_for_backward(pred, target, t, masks, w)
        return out[0]

    @staticmethod
    def backward(ctx, dloss):
        pred, target, t, masks, w = ctx.saved_tensors
        d = ctx.seeded.take(dloss)
        if d is None:
            _, d = K.diffusion_loss(pred, target, t, w, ctx.scale, masks=masks, seed=dloss.reshape(1).float().contiguous(), grad=True,
                                    dpred=ctx.seeded.spare())
        return d, None, None, None, None, None, None


def _diffusion_weights(schedule, device):
    """The fp32 table sqrt(snr + 1) for the `sample` objective, None for `epsilon` (weight 1)."""
    return schedule.on(device).w if schedule.prediction_type == "sample" else None


def diffusion_loss(pred, target, t, schedule, masks=None, scale=1.0, seed=None):
    """-> the fp32 loss scale * mean_b(sum_t(!mask * mean_d |w_b (pred - target)|) / sum_t(!mask)).  pred [B, T, max_data_dim]: the frame
    decoder's rows in the model dtype, read in place at the target's columns; target fp32 [B, T, Dd]: x0 for the `sample` objective
    (w_b = sqrt(snr(t_b) + 1)), the noise for `epsilon` (w_b = 1); t int64 [B]; masks bool [B, T] (True: padding) or None."""
    return DiffusionLossFn.apply(pred, target, t, masks, _diffusion_weights(schedule, pred.device), float(scale), seed)


def diffusion_eval(pred, target, t, schedule, masks=None, scale=1.0):
    """The validation form: the same launch without the gradient -> fp32 [1]."""
    return K.diffusion_loss(pred, target, t, _diffusion_weights(schedule, pred.device), scale, masks=masks)[0]


# ---------------------------------------------------------------------------------------------- speech generation (csrc/speech_step.hip)
def speech_step_fusable(x_dtype, head, prenet, proj):
    """Can ofa_speech_step serve these weights: a served shape (K.speech_step_ok) and contiguous, 16-byte aligned tensors of one dtype?"""
    feat_w, feat_b, eos_w, eos_b = head
    tensors = [feat_w, feat_b, eos_w, eos_b, proj[0], proj[1]] + [t for wb in prenet for t in wb]
    if not prenet or any(t.dtype != x_dtype or not t.is_contiguous() for t in tensors):
        return False
    if any(t.data_ptr() % 16 for t in (feat_w, eos_w, proj[0]) + tuple(w for w, _ in prenet)):
        return False
    return K.speech_step_ok(feat_w.shape[1], feat_w.shape[0], proj[0].shape[1], proj[0].shape[0], len(prenet), x_dtype)


def speech_step(x, head, prenet, proj, state, step, p_drop, fused=True):
    """Everything an autoregressive speech-generation step does after the decoder (generator/speech_generator.py:155-166 and the next
    step's adaptor/audio.py:327-336 prenet), on the device, without a host synchronisation; inference only.  x [B, D]: the decoder's
    output at the new position; head = (feat_w, feat_b, eos_w, eos_b), prenet = [(w, b), ...], proj = (w, b): the adaptor's Linear
    parameters, read in place; state: kernels.speech_step's buffers.  fused: ONE launch (ofa_speech_step); else the unfused composition
    of the existing kernels (linear / relu / dropout_add) and small torch ops on the state -- the same roundings and the same dropout
    masks (both reserve the Philox positions of one [B, prenet_dim] dropout per layer, in layer order), so the two differ in the summation
    order of the dot products alone."""
    B = x.shape[0]
    P = proj[0].shape[1]
    if fused:
        seed = off0 = stride = 0
        base = None
        if p_drop > 0:
            offs = [_Rng.reserve(B * P, x.device) for _ in prenet]
            seed, off0, base = offs[0]
            stride = offs[1][1] - off0 if len(offs) > 1 else 0
            assert all(o[1] == off0 + i * stride for i, o in enumerate(offs))
        K.speech_step(x, head, prenet, proj, state, step, p_drop, seed, off0, stride, base)
        return
    feat_w, feat_b, eos_w, eos_b = head
    feat = linear(x, feat_w, feat_b)
    # (eos_proj has one output row: the GEMM runs 8 wide on zero-padded copies, as the training head does)
    eos = linear(x, torch.nn.functional.pad(eos_w, (0, 0, 0, 7)), torch.nn.functional.pad(eos_b, (0, 7)))[:, 0]
    p = torch.sigmoid(eos.float())
    state["feats"][:, step].copy_(feat)
    state["eos_prob"][:, step].copy_(p)
    was = state["finished"].ne(0)
    cross = p > state["threshold"]                                        # (fp32 [1] on the device: no threshold in a captured step)
    newly = cross & ~was
    state["out_lens"].masked_fill_(newly, step + 1)
    state["nfin"].add_(newly.sum().to(torch.int32))
    fin = was | cross
    state["finished"].copy_(fin)
    state["pad_next"].view(-1).copy_(fin)
    h = feat
    for w, b in prenet:
        h = dropout_add(relu(linear(h, w, b)), None, p_drop, True)
    state["embed"].copy_(linear(h, proj[0], proj[1]))
