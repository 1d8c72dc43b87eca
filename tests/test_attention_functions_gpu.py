"""GPU: the autograd Functions in front of the fused attention kernels (ofasys_amd.ops: PackedSelfAttentionFn, InProjSelfAttentionFn,
PackedCrossAttentionFn, CrossKVShared), called directly with the modules' parameters and `m._pack`.

Mode A -- no FlatParams, no gradient sinks: every output of a Function (out, the input gradients, every weight / bias gradient, dbias,
the c_attn gradient) equals, BIT FOR BIT, the same computation written here from dense primitives (dense_self / dense_cross: K.gemm of the
concatenated weight, contiguous q / k / v, K.attn_fwd / K.attn_bwd with dense outputs, the concatenated d buffer, K.gemm for dx and dW,
K.colsum for db, K.c_attn_grad).  tests/test_attention_edges_gpu.py pins packed layouts as bit-identical to dense ones and the GEMMs see
the same operands, so equality is exact.

Mode B -- trainer.FlatParams over the modules, gradient arena zeroed, once with ops.defer_reductions(False) and once with True:
  * out, the input gradients and dbias equal the dense computation (hence mode A) bit for bit;
  * autograd receives None for every sunk parameter, p.grad still points into the arena, and every sunk parameter the call uses
    reports `_ofa_grad_ready` exactly once (everything else: never) by the time backward() returns;
  * every arena gradient g is within  eps(g.dtype) |s| + n 2^-23 sum|terms|  of the float64 sum s of its n terms (columns of the d
    buffer for a bias; the products d * x, exact in fp32 for 16-bit operands, for a weight): an fp32 accumulation in any order plus
    one rounding to the arena's dtype (the epilogue-served bias gradients: plus SLACK, see there);
  * the c_attn gradient is within test_kernels_gpu.py::test_c_attn_grad_kernel's tolerance (its out= / accumulate form, which is what
    the arena receives) of mode A's;
  * the stack-wide k|v projection (CrossKVShared) with both layers in it, and with one layer kept out.
Ragged (Segments) inputs stay with tests/test_packing_gpu.py."""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
DT = torch.bfloat16
B, HEADS, D = 2, 2, 128
SCALE = float(64 * 2) ** -0.5
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
C_ATTN_TOL = 1.6e-2                      # test_c_attn_grad_kernel, 16-bit, the out= / accumulate=True call
# The bias gradients that the attention backward's epilogues serve do not meet the bound above as it stands: the epilogues sum the
# kernels' fp32 dq / dk / dv BEFORE these are rounded to 16 bits, so every term differs from the d buffer's entry by up to half an ulp
# (at most 2^-9 sum|terms| in all).  Measured on the code before the Functions shared their backward helpers, over every case of this
# file, the largest (error - bound) / sum|terms| was: self db 8.229e-4 (e.g. T = 33, no bias: element 116, error 3.46e-3 against a
# bound of 5.3e-5), in_proj db 6.972e-4, cross dbq 7.115e-4, the stack-wide b_all 8.158e-4; every other gradient -- all weights, and the
# biases that take the colsum pass -- stays inside the bound (error / bound <= 0.992).  Those four get TWICE that excess, as a multiple of
# sum|terms|, on top of the bound; nothing else gets any.
SLACK = {"self db": 2 * 8.229e-4, "in_proj db": 2 * 6.972e-4, "cross dbq": 2 * 7.115e-4, "b_all": 2 * 8.158e-4}

# (T, bias, key padding, c_attn, causal)
SELF_CASES = [(33, None, False, False, False), (33, "dense", True, True, False), (33, "shared", True, False, False),
              (129, None, True, True, False), (129, "dense", False, False, False), (129, "shared", False, True, True)]
# (T, S, bias, key padding, c_attn)
CROSS_CASES = [(33, 97, None, False, False), (33, 97, "dense", True, True), (33, 97, "shared", False, True),
               (129, 33, None, True, True), (129, 33, "dense", False, False), (129, 33, "shared", True, False)]
IN_PROJ_T = [33, 129]


def _id(case):
    return "-".join(str(c) for c in case)


# ------------------------------------------------------------------------------------------------------------------ modules and inputs
def build_modules():
    """self-attention, two encoder-decoder attentions (so that FlatParams builds `_cross_all`) and the ViT in_proj form: the same values
    on every call."""
    from ofasys_amd.module.multihead_attention import MultiheadAttention
    from ofasys_amd.module.vit import InProjSelfAttention
    torch.manual_seed(1234)
    mods = torch.nn.ModuleDict({
        "self": MultiheadAttention(D, HEADS, self_attention=True, scale_heads=True),
        "cross0": MultiheadAttention(D, HEADS, encoder_decoder_attention=True, scale_heads=True),
        "cross1": MultiheadAttention(D, HEADS, encoder_decoder_attention=True, scale_heads=True),
        "vit": InProjSelfAttention(D, HEADS),
    })
    with torch.no_grad():
        for n, p in mods.named_parameters():
            if p.dim() == 1:                                     # biases: not all zero; c_attn: around one
                p.copy_(torch.rand(p.shape) + 0.5 if n.endswith("c_attn") else 0.25 * torch.randn(p.shape))
    return mods.to(device=DEV, dtype=DT)


def _randn(g, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=g)).to(device=DEV, dtype=DT)


def make_inputs(seed, T, S, bias, kpm):
    """x [B,T,D], enc [B,S,D], dout [B,T,D] (two of each: one per cross layer), bias tensor or None, key-padding mask or None.  The
    mask pads sample 1 from three keys before the last 32-key boundary to the end, so it crosses that boundary."""
    g = torch.Generator().manual_seed(seed)
    x = [_randn(g, B, T, D), _randn(g, B, T, D)]
    enc = _randn(g, B, S, D)
    dout = [_randn(g, B, T, D), _randn(g, B, T, D)]
    bt = None
    if bias == "dense":
        bt = [_randn(g, B * HEADS, T, S, scale=0.5) for _ in range(2)]
    elif bias == "shared":
        bt = [_randn(g, HEADS, T, S, scale=0.5) for _ in range(2)]
    mask = None
    if kpm:
        mask = torch.zeros(B, S, dtype=torch.bool)
        mask[1, S - S % 32 - 3:] = True
        mask = mask.to(DEV)
    return x, enc, dout, bt, mask


def shared_arg(bias, t):
    """-> (bias tensor handed to the Function, its bias_shared argument)."""
    from ofasys_amd import ops
    if bias != "shared":
        return t, False
    return t, ops.SharedBias.of(t).shared_arg()


# ------------------------------------------------------------------------------------------------------------------ the dense computation
def _attn_dense(K, q, k, v, dout, bias, shared, mask, c, causal):
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    out, lse = K.attn_fwd(q, k, v, HEADS, SCALE, bias=bias, kpm=mask, c_attn=c, causal=causal, bias_shared=shared)
    dq, dk, dv, dbias, delta = K.attn_bwd(q, k, v, out, dout, lse, HEADS, SCALE, bias=bias, kpm=mask, c_attn=c, causal=causal,
                                          need_dbias=bias is not None, bias_shared=shared,
                                          dbias_dtype=bias.dtype if (shared and bias is not None) else torch.float32)
    if dbias is not None and shared:
        dbias = dbias.view(bias.shape)
    dc = K.c_attn_grad(delta, c, q.shape[0], HEADS, q.shape[1]) if c is not None else None
    return out, dq, dk, dv, dbias, dc


def _proj_dense(K, d2, x2, W):
    """-> dx, dW, db of y = x W^T + b given d2 = dy."""
    return K.gemm(d2, W, False, False), K.gemm(d2, x2, True, False), K.colsum(d2, out_dtype=d2.dtype)


def dense_self(K, ws, bs, order, x, dout, bias, shared, mask, c, causal):
    """ws / bs: the three weights / biases in the pack's column order `order` ("kvq" or "qkv").  -> dict of every output, the d buffer
    and x2."""
    T = x.shape[1]
    W, bv = torch.cat(ws), torch.cat(bs)
    x2 = x.reshape(B * T, D)
    y = K.gemm(x2, W, False, True, bias=bv).view(B, T, 3 * D)
    col = {n: y[:, :, i * D:(i + 1) * D] for i, n in enumerate(order)}
    out, dq, dk, dv, dbias, dc = _attn_dense(K, col["q"], col["k"], col["v"], dout, bias, shared, mask, c, causal)
    dcol = {"q": dq, "k": dk, "v": dv}
    d2 = torch.cat([dcol[n] for n in order], dim=-1).view(B * T, 3 * D)
    dx, dW, db = _proj_dense(K, d2, x2, W)
    return dict(out=out, dx=dx.view(B, T, D), dW=dW, db=db, dbias=dbias, dc=dc, d2=d2, x2=x2)


def dense_cross(K, m, xq, enc, dout, bias, shared, mask, c):
    T, S = xq.shape[1], enc.shape[1]
    wq, bq = m.q_proj.weight.detach(), m.q_proj.bias.detach()
    W = torch.cat([m.k_proj.weight.detach(), m.v_proj.weight.detach()])
    bv = torch.cat([m.k_proj.bias.detach(), m.v_proj.bias.detach()])
    xq2, xkv2 = xq.reshape(B * T, D), enc.reshape(B * S, D)
    q = K.gemm(xq2, wq, False, True, bias=bq).view(B, T, D)
    kv = K.gemm(xkv2, W, False, True, bias=bv).view(B, S, 2 * D)
    out, dq, dk, dv, dbias, dc = _attn_dense(K, q, kv[:, :, :D], kv[:, :, D:], dout, bias, shared, mask, c, False)
    dq2, dkv2 = dq.view(B * T, D), torch.cat([dk, dv], dim=-1).view(B * S, 2 * D)
    dxq, dWq, dbq = _proj_dense(K, dq2, xq2, wq)
    dxkv, dWkv, dbkv = _proj_dense(K, dkv2, xkv2, W)
    return dict(out=out, dxq=dxq.view(B, T, D), dxkv=dxkv.view(B, S, D), dWq=dWq, dbq=dbq, dWkv=dWkv, dbkv=dbkv, dbias=dbias, dc=dc,
                dq2=dq2, dkv2=dkv2, xq2=xq2, xkv2=xkv2)


_REF = {}


def reference(key, make):
    """The dense computation of a case: computed once, shared by the tests of both modes, never written to."""
    if key not in _REF:
        with torch.no_grad():
            _REF[key] = make()
        torch.cuda.synchronize()
    return _REF[key]


def ref_self(K, case):
    T, bias, kpm, c, causal = case

    def make():
        m = build_modules()["self"]
        x, _, dout, bt, mask = make_inputs(11, T, T, bias, kpm)
        b, shared = shared_arg(bias, bt[0] if bt else None)
        ps = [p.detach() for p in (m.k_proj.weight, m.v_proj.weight, m.q_proj.weight, m.k_proj.bias, m.v_proj.bias, m.q_proj.bias)]
        return dense_self(K, ps[:3], ps[3:], "kvq", x[0], dout[0], b, shared, mask, m.c_attn.detach() if c else None, causal)
    return reference(("self",) + tuple(case), make)


def ref_in_proj(K, T):
    def make():
        m = build_modules()["vit"]
        x, _, dout, _, _ = make_inputs(13, T, T, None, False)
        w, b = m.in_proj_weight.detach(), m.in_proj_bias.detach()
        r = dense_self(K, [w[i * D:(i + 1) * D] for i in range(3)], [b[i * D:(i + 1) * D] for i in range(3)], "qkv", x[0], dout[0],
                       None, False, None, None, False)
        r["db"] = K.colsum(r["d2"], out_dtype=b.dtype)       # (the in_proj form returns the bias gradient in the parameter's dtype)
        return r
    return reference(("in_proj", T), make)


def ref_cross(K, case):
    """-> [layer 0's dict, layer 1's dict]: two layers with their own query streams, biases and parameters over ONE encoder output."""
    T, S, bias, kpm, c = case

    def make():
        mods = build_modules()
        x, enc, dout, bt, mask = make_inputs(17, T, S, bias, kpm)
        refs = []
        for i in range(2):
            m = mods["cross%d" % i]
            b, shared = shared_arg(bias, bt[i] if bt else None)
            refs.append(dense_cross(K, m, x[i], enc, dout[i], b, shared, mask, m.c_attn.detach() if c else None))
        return refs
    return reference(("cross",) + tuple(case), make)


# ------------------------------------------------------------------------------------------------------------------ calling the Functions
def call_self(ops, m, x, bias, shared, mask, c, causal):
    return ops.PackedSelfAttentionFn.apply(x, m.k_proj.weight, m.v_proj.weight, m.q_proj.weight, m.k_proj.bias, m.v_proj.bias,
                                           m.q_proj.bias, bias, mask, c, HEADS, SCALE, causal, m._pack, shared)


def call_cross(ops, m, xq, xkv, bias, shared, mask, c, kv_all=None, layer=0):
    return ops.PackedCrossAttentionFn.apply(xq, xkv, m.k_proj.weight, m.v_proj.weight, m.q_proj.weight, m.k_proj.bias, m.v_proj.bias,
                                            m.q_proj.bias, bias, mask, c, HEADS, SCALE, m._pack, shared, kv_all, layer)


def leaf(t):
    return t.detach().clone().requires_grad_(True) if t is not None else None


def same(got, want, tag):
    assert (got is None) == (want is None), (tag, "one side is None")
    if want is not None:
        assert got.shape == want.shape and got.dtype == want.dtype, (tag, tuple(got.shape), got.dtype, tuple(want.shape), want.dtype)
        assert torch.equal(got, want), (tag, "differs in %d elements" % int((got != want).sum()))


# ------------------------------------------------------------------------------------------------------------------ mode A
@pytest.fixture(scope="module")
def K():
    from ofasys_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def ops():
    from ofasys_amd import ops
    return ops


@pytest.mark.parametrize("case", SELF_CASES, ids=_id)
def test_self_mode_a(K, ops, case):
    T, bias, kpm, c, causal = case
    ref = ref_self(K, case)
    m = build_modules()["self"]
    xs, _, dout, bt, mask = make_inputs(11, T, T, bias, kpm)
    x, b = leaf(xs[0]), leaf(bt[0] if bt else None)
    bb, shared = shared_arg(bias, b)
    out = call_self(ops, m, x, bb, shared, mask, m.c_attn if c else None, causal)
    out.backward(dout[0])
    same(out.detach(), ref["out"], "out")
    same(x.grad, ref["dx"], "dx")
    same(b.grad if b is not None else None, ref["dbias"], "dbias")
    same(torch.cat([m.k_proj.weight.grad, m.v_proj.weight.grad, m.q_proj.weight.grad]), ref["dW"], "dW")
    same(torch.cat([m.k_proj.bias.grad, m.v_proj.bias.grad, m.q_proj.bias.grad]), ref["db"], "db")
    same(m.c_attn.grad, ref["dc"], "dc")


@pytest.mark.parametrize("T", IN_PROJ_T)
def test_in_proj_mode_a(K, ops, T):
    ref = ref_in_proj(K, T)
    m = build_modules()["vit"]
    xs, _, dout, _, _ = make_inputs(13, T, T, None, False)
    x = leaf(xs[0])
    out = ops.InProjSelfAttentionFn.apply(x, m.in_proj_weight, m.in_proj_bias, HEADS, SCALE)
    out.backward(dout[0])
    same(out.detach(), ref["out"], "out")
    same(x.grad, ref["dx"], "dx")
    same(m.in_proj_weight.grad, ref["dW"], "dW")
    same(m.in_proj_bias.grad, ref["db"], "db")


@pytest.mark.parametrize("case", CROSS_CASES, ids=_id)
def test_cross_mode_a(K, ops, case):
    T, S, bias, kpm, c = case
    refs = ref_cross(K, case)
    mods = build_modules()
    xs, enc0, dout, bt, mask = make_inputs(17, T, S, bias, kpm)
    for i in range(2):
        m, ref = mods["cross%d" % i], refs[i]
        xq, enc, b = leaf(xs[i]), leaf(enc0), leaf(bt[i] if bt else None)
        bb, shared = shared_arg(bias, b)
        out = call_cross(ops, m, xq, enc, bb, shared, mask, m.c_attn if c else None)
        out.backward(dout[i])
        same(out.detach(), ref["out"], "out")
        same(xq.grad, ref["dxq"], "dxq")
        same(enc.grad, ref["dxkv"], "dxkv")
        same(b.grad if b is not None else None, ref["dbias"], "dbias")
        same(m.q_proj.weight.grad, ref["dWq"], "dWq")
        same(m.q_proj.bias.grad, ref["dbq"], "dbq")
        same(torch.cat([m.k_proj.weight.grad, m.v_proj.weight.grad]), ref["dWkv"], "dWkv")
        same(torch.cat([m.k_proj.bias.grad, m.v_proj.bias.grad]), ref["dbkv"], "dbkv")
        same(m.c_attn.grad, ref["dc"], "dc")


# ------------------------------------------------------------------------------------------------------------------ mode B
class Arena:
    """The modules under trainer.FlatParams with a zeroed gradient arena, counting `_ofa_grad_ready` per parameter and recording every
    parameter autograd delivers a gradient to."""

    def __init__(self, ops, defer):
        from ofasys_amd.trainer import FlatParams
        self.ops = ops
        self.mods = build_modules()
        self.fp = FlatParams(self.mods)
        self.fp.grad.zero_()
        self.names = {id(p): n for n, p in self.mods.named_parameters()}
        self.ready = {n: 0 for n in self.names.values()}
        self.delivered = []
        for p in self.fp.params:
            n = self.names[id(p)]
            p._ofa_grad_ready = lambda n=n: self.ready.__setitem__(n, self.ready[n] + 1)
            p.register_hook(lambda g, n=n: self.delivered.append(n) if g is not None else None)
        self.prev = ops._Fold.queue is not None
        ops.drop_pending()
        ops.defer_reductions(defer)

    def close(self):
        try:
            self.ops.defer_reductions(self.prev)
        finally:
            self.ops.drop_pending()

    def check_bookkeeping(self, used):
        """`used`: the parameters (names) the call sinks gradients into."""
        torch.cuda.synchronize()
        assert self.delivered == [], ("autograd received a gradient for sunk parameters", self.delivered)
        lo, hi = self.fp.grad.data_ptr(), self.fp.grad.data_ptr() + self.fp.grad.numel() * self.fp.grad.element_size()
        for p in self.fp.params:
            assert p.grad is not None and p.grad.data_ptr() == p._ofa_grad.data_ptr() and lo <= p.grad.data_ptr() < hi, self.names[id(p)]
        want = {n: int(n in used) for n in self.ready}
        assert self.ready == want, {n: (self.ready[n], want[n]) for n in want if self.ready[n] != want[n]}

    def check_unused_zero(self, used):
        for p in self.fp.params:
            if self.names[id(p)] not in used:
                assert not bool(p.grad.any()), (self.names[id(p)], "an unused parameter's arena gradient was written")


def within_bound(g, d2, x2, tag, slack=0.0):
    """g: an arena gradient; the float64 sum s of its terms -- columns of d2 (x2 None: a bias) or the products d2^T x2 (a weight) --
    with |g - s| <= eps(g.dtype) |s| + n 2^-23 sum|terms| + slack sum|terms|, n = rows of d2 (slack: see EPILOGUE_SLACK)."""
    dd = d2.double()
    if x2 is None:
        s, a = dd.sum(0), dd.abs().sum(0)
    else:
        s, a = dd.t() @ x2.double(), dd.abs().t() @ x2.double().abs()
    n = d2.shape[0]
    err = (g.double().reshape(s.shape) - s).abs()
    bound = EPS[g.dtype] * s.abs() + n * 2.0 ** -23 * a
    over = err - bound
    print("BOUND", tag, "largest error / bound %.3f, largest excess / sum|terms| %.3e"
          % (float((err / bound.clamp_min(1e-300)).max()), float((over / a.clamp_min(1e-300)).max())))
    over = over - slack * a
    i = int(over.argmax())
    assert float(over.max()) <= 0.0, (tag, "element", i, "error", float(err.reshape(-1)[i]), "bound", float(bound.reshape(-1)[i]),
                                      "sum|terms|", float(a.reshape(-1)[i]))


def c_attn_close(g, want, tag):
    r = float((g.double() - want.double()).abs().max() / want.double().abs().max().clamp_min(1e-30))
    print(tag, "c_attn rel %.2e" % r)
    assert r < C_ATTN_TOL, (tag, r)


def pnames(prefix, which):
    table = {"k": ("k_proj.weight", "k_proj.bias"), "v": ("v_proj.weight", "v_proj.bias"), "q": ("q_proj.weight", "q_proj.bias"),
             "c": ("c_attn",)}
    return {prefix + "." + n for w in which for n in table[w]}


@pytest.mark.parametrize("defer", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("case", SELF_CASES, ids=_id)
def test_self_mode_b(K, ops, case, defer):
    T, bias, kpm, c, causal = case
    ref = ref_self(K, case)
    a = Arena(ops, defer)
    try:
        m = a.mods["self"]
        assert {"w", "b", "gw", "gb"} <= set(m._pack)
        xs, _, dout, bt, mask = make_inputs(11, T, T, bias, kpm)
        x, b = leaf(xs[0]), leaf(bt[0] if bt else None)
        bb, shared = shared_arg(bias, b)
        out = call_self(ops, m, x, bb, shared, mask, m.c_attn if c else None, causal)
        out.backward(dout[0])
        used = pnames("self", "kvqc" if c else "kvq")
        a.check_bookkeeping(used)
        same(out.detach(), ref["out"], "out")
        same(x.grad, ref["dx"], "dx")
        same(b.grad if b is not None else None, ref["dbias"], "dbias")
        within_bound(torch.cat([m.k_proj.weight.grad, m.v_proj.weight.grad, m.q_proj.weight.grad]), ref["d2"], ref["x2"], "dW")
        within_bound(torch.cat([m.k_proj.bias.grad, m.v_proj.bias.grad, m.q_proj.bias.grad]), ref["d2"], None, "self db", SLACK["self db"])
        if c:
            c_attn_close(m.c_attn.grad, ref["dc"], "self")
        a.check_unused_zero(used)
    finally:
        a.close()


@pytest.mark.parametrize("defer", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("T", IN_PROJ_T)
def test_in_proj_mode_b(K, ops, T, defer):
    ref = ref_in_proj(K, T)
    a = Arena(ops, defer)
    try:
        m = a.mods["vit"]
        xs, _, dout, _, _ = make_inputs(13, T, T, None, False)
        x = leaf(xs[0])
        out = ops.InProjSelfAttentionFn.apply(x, m.in_proj_weight, m.in_proj_bias, HEADS, SCALE)
        out.backward(dout[0])
        used = {"vit.in_proj_weight", "vit.in_proj_bias"}
        a.check_bookkeeping(used)
        same(out.detach(), ref["out"], "out")
        same(x.grad, ref["dx"], "dx")
        within_bound(m.in_proj_weight.grad, ref["d2"], ref["x2"], "dW")
        within_bound(m.in_proj_bias.grad, ref["d2"], None, "in_proj db", SLACK["in_proj db"])
        a.check_unused_zero(used)
    finally:
        a.close()


def _cross_arena_grads(mods, refs, layers, tag, kv_slack=0.0):
    """The arena gradients of the cross-attention layers `layers` against the bound (kv_slack: the k | v biases came from the epilogues)."""
    for i in layers:
        m, ref = mods["cross%d" % i], refs[i]
        within_bound(m.q_proj.weight.grad, ref["dq2"], ref["xq2"], "%s dWq%d" % (tag, i))
        within_bound(m.q_proj.bias.grad, ref["dq2"], None, "%s dbq%d" % (tag, i), SLACK["cross dbq"])
        within_bound(torch.cat([m.k_proj.weight.grad, m.v_proj.weight.grad]), ref["dkv2"], ref["xkv2"], "%s dWkv%d" % (tag, i))
        within_bound(torch.cat([m.k_proj.bias.grad, m.v_proj.bias.grad]), ref["dkv2"], None, "%s dbkv%d" % (tag, i), kv_slack)


@pytest.mark.parametrize("defer", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("case", CROSS_CASES, ids=_id)
def test_cross_stack_wide_kv(K, ops, case, defer):
    """Both layers read and write their slice of ONE k|v projection: dkv_all's slices are mode A's per-layer dk|dv, the encoder gradient
    comes back through layer 0 only as K.gemm(dkv_all, W_all), W_all / b_all meet the bound, all 4 + 4 (+ q, c_attn) parameters report once."""
    T, S, bias, kpm, c = case
    refs = ref_cross(K, case)
    a = Arena(ops, defer)
    try:
        mods = a.mods
        pack = mods["cross0"]._cross_all[0]
        assert mods["cross1"]._cross_all == (pack, 1) and pack["layers"] == 2
        xs, enc0, dout, bt, mask = make_inputs(17, T, S, bias, kpm)
        enc = leaf(enc0)
        kvs = ops.CrossKVShared(enc.detach().view(B * S, D), pack)
        xq = [leaf(xs[0]), leaf(xs[1])]
        bl = [leaf(bt[i] if bt else None) for i in range(2)]
        outs = []
        for i in range(2):                                  # (layer 0's node is created first: it runs last in backward)
            m = mods["cross%d" % i]
            bb, shared = shared_arg(bias, bl[i])
            outs.append(call_cross(ops, m, xq[i], enc if i == 0 else None, bb, shared, mask, m.c_attn if c else None, kvs, i))
        torch.autograd.backward(outs, [dout[0], dout[1]])
        used = pnames("cross0", "kvqc" if c else "kvq") | pnames("cross1", "kvqc" if c else "kvq")
        a.check_bookkeeping(used)
        for i in range(2):
            same(outs[i].detach(), refs[i]["out"], "out%d" % i)
            same(xq[i].grad, refs[i]["dxq"], "dxq%d" % i)
            same(bl[i].grad if bl[i] is not None else None, refs[i]["dbias"], "dbias%d" % i)
            same(kvs.dkv_all[:, i * 2 * D:(i + 1) * 2 * D].contiguous(), refs[i]["dkv2"], "dkv_all slice %d" % i)
        same(enc.grad, K.gemm(kvs.dkv_all, pack["w"], False, False).view(B, S, D), "d enc")
        _cross_arena_grads(mods, refs, (0, 1), "stack-wide", SLACK["b_all"])
        dall = torch.cat([refs[0]["dkv2"], refs[1]["dkv2"]], dim=1)
        within_bound(pack["gw"], dall, refs[0]["xkv2"], "W_all")
        within_bound(pack["gb"], dall, None, "b_all", SLACK["b_all"])
        if c:
            for i in range(2):
                c_attn_close(mods["cross%d" % i].c_attn.grad, refs[i]["dc"], "cross%d" % i)
        a.check_unused_zero(used)
    finally:
        a.close()


@pytest.mark.parametrize("defer", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("case", CROSS_CASES, ids=_id)
def test_cross_one_layer_stays_out(K, ops, case, defer):
    """Layer 1 keeps its own projection (kv_all=None, its parameters report through its own backward); layer 0 alone uses the stack-wide
    one, so CrossKVShared.finish touches only layer 0's slices."""
    T, S, bias, kpm, c = case
    refs = ref_cross(K, case)
    a = Arena(ops, defer)
    try:
        mods = a.mods
        pack = mods["cross0"]._cross_all[0]
        xs, enc0, dout, bt, mask = make_inputs(17, T, S, bias, kpm)
        enc = leaf(enc0)
        kvs = ops.CrossKVShared(enc.detach().view(B * S, D), pack)
        xq = [leaf(xs[0]), leaf(xs[1])]
        bl = [leaf(bt[i] if bt else None) for i in range(2)]
        outs = []
        for i in range(2):
            m = mods["cross%d" % i]
            bb, shared = shared_arg(bias, bl[i])
            outs.append(call_cross(ops, m, xq[i], enc, bb, shared, mask, m.c_attn if c else None, kvs if i == 0 else None, i))
        torch.autograd.backward(outs, [dout[0], dout[1]])
        used = pnames("cross0", "kvqc" if c else "kvq") | pnames("cross1", "kvqc" if c else "kvq")
        a.check_bookkeeping(used)
        for i in range(2):
            same(outs[i].detach(), refs[i]["out"], "out%d" % i)
            same(xq[i].grad, refs[i]["dxq"], "dxq%d" % i)
            same(bl[i].grad if bl[i] is not None else None, refs[i]["dbias"], "dbias%d" % i)
        same(kvs.dkv_all[:, :2 * D].contiguous(), refs[0]["dkv2"], "dkv_all slice 0")
        assert not bool(kvs.dkv_all[:, 2 * D:].any()), "the slice of the layer that stayed out must be zero"
        # the encoder output's gradient: layer 0's node (the whole-stack GEMM over a zero slice) and layer 1's own, met by autograd
        d0 = K.gemm(kvs.dkv_all, pack["w"], False, False).view(B, S, D)
        same(enc.grad, d0 + refs[1]["dxkv"], "d enc")
        _cross_arena_grads(mods, refs, (0, 1), "one out")
        if c:
            for i in range(2):
                c_attn_close(mods["cross%d" % i].c_attn.grad, refs[i]["dc"], "cross%d" % i)
        a.check_unused_zero(used)
    finally:
        a.close()
