"""The (entry point, dtype) cells of the C ABI that no other GPU test launches, once each.

Every entry point of csrc/*.hip turns its runtime dtype into the kernel's template argument through dispatch_dtype (csrc/common.h):
one launch written with T, (const T*)x and Vec<T>::N.  What a comparison of the device assembly cannot see is a host-side slip in ONE
dtype's instantiation, so each case here runs one entry point in one dtype the rest of the suite leaves out (GAPS, from the table
below), at the smallest shape that still takes the 16-byte vector path and its
tail: 3 to 5 rows, 40 columns for the 16-bit types and 20 for fp32 (whole vectors, no power of two), an odd width where an entry point
has a scalar fallback.  References are fp32 torch on the same already-rounded inputs; tolerances are the ones the existing test of the
same entry point uses for that dtype (fp16 without a precedent: the bf16 one), integer-indexed moves compare bit for bit.

Who launches what (read off the suite; k = tests/test_kernels_gpu.py, h = test_fp16_gpu.py, e = test_step_edges_gpu.py,
s = test_attn_sbias_gpu.py, a = test_attnside_edges_gpu.py, m = the model / train-step suites (fp32 and bf16; fp16 through h's two model tests, which are not counted
as covering a cell); NEW = a case of this file):

  entry point(s)                                    fp32                 bf16                 fp16
  layernorm_fwd/bwd, gelu_layernorm_fwd/bwd         k test_layernorm     k test_layernorm     h test_layernorm_fp16
  scaled_* softmax fwd/bwd (three families)         k test_softmax_family (all three dtypes); per element: a (all three)
  attn_softmax_fwd                                  k test_attn_softmax  k test_attn_softmax  NEW; per element: a (all three)
  gemm (simple kernel)                              k test_gemm          k test_gemm          h test_gemm_fp16
  gelu_fwd/bwd, dropout_add_fwd/bwd, add_rowvec_mask  k test_elementwise k test_elementwise   NEW
  embedding_fwd (vector kernel)                     k test_embedding     k test_embedding     h test_embedding_criterion_adam_fp16
  embedding_fwd (scalar kernel, odd width)          NEW                  NEW                  NEW
  embedding_bwd, embedding_bwd_ids                  e test_token_backward_id_major_equals_row_major (all three)
  embedding_range_bwd, batch_sum                    e test_position_range_backward_equals_batch_sum_and_scatter (all three)
  im2col_patch                                      e test_im2col_patch_equals_unfold (all three)
  gather_rows                                       NEW                  s ragged-attention packing  NEW
  gather_rows_parts, scatter_rows_part              NEW                  test_packing_gpu     NEW
  segment_rowsum                                    s test_planned_table_gradient_...  (same)  NEW
  colsum (operand / output type)                    NEW                  e test_queued_column_sums_equal_immediate_ones  NEW
  add_n                                             k test_add_n_and_fan_out (all three)
  mul                                               NEW                  m                    NEW
  scale_row_groups                                  k test_drop_path_per_sample  (same)       NEW
  im2col, col2im                                    k test_conv2d        k test_conv2d        h test_conv_batchnorm_fp16; NHWC<-NCHW gather: NEW
  batchnorm_fwd, batchnorm_bwd                      k test_batchnorm     k test_batchnorm     h test_conv_batchnorm_fp16
  batchnorm_fwd_stats/_fwd_apply/_bwd_stats/_bwd_dx test_syncbn_gpu      test_syncbn_gpu      NEW (fwd_apply also k test_conv_bn_statistics_...)
  maxpool_fwd/bwd, relu                             k test_maxpool_relu  k test_maxpool_relu  NEW
  cross_entropy_fwd/bwd                             k test_cross_entropy k test_cross_entropy NEW
  cross_entropy_fwd_grad (16-bit only)              -                    k test_cross_entropy_forward_and_gradient_in_one_pass (both)
  ls_cross_entropy_fwd/bwd                          k test_label_smoothed_cross_entropy (fp32, bf16)  h test_embedding_criterion_adam_fp16
  probs_fwd/bwd                                     NEW                  NEW (fwd: test_model_gpu test_get_normalized_probs_and_train_mode)  NEW
  sumsq                                             k test_adam_and_sumsq  k test_adam_and_sumsq  h test_embedding_criterion_adam_fp16
  adam_step                                         NEW                  k test_adam_and_sumsq  h test_embedding_criterion_adam_fp16
  bias_block_add/_add_batch/_slice/_grad            NEW                  m                    NEW; per element: a (all three)
  bias_outer_grad                                   NEW                  s test_bias_build_outer_slot_and_its_gradient  NEW; exact: a (all three)
  bias_build (16-bit only)                          -                    s test_bias_build_assembles_and_swizzles  NEW; a (both)
  join_fwd                                          k test_residual_join_equals_unfused_chain (fp32, bf16)  h test_residual_join_fp16
  join_bwd                                          k (same)             k (same)             NEW
  beam_topk, beam_prefix_topk, trie_beam_topk, closed_set_edge_logits   test_beam_search_gpu / test_beam_prefix_gpu / test_trie_beam_gpu / test_traverse_gpu (all three)
  attn_decode                                       k test_attn_decode_matches_reference (fp32, bf16)  NEW; per element: a (all three)
  attn_bwd_prep (16-bit only)                       -                    k test_fused_attention  h test_fused_attention_fp16; a (both)
  mean_heads                                        NEW                  m                    NEW; per element: a (all three)
  c_attn_grad                                       k test_c_attn_grad_kernel (fp32, bf16)    NEW; exact: a (all three)
  transpose_heads                                   a test_transpose_heads_bit_for_bit (all three)"""
import pytest
import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import rel, tol

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF, H = torch.float32, torch.bfloat16, torch.float16


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ofasys_amd import kernels
    return kernels


def cols_of(dtype):
    return 20 if dtype == F32 else 40


def rnd(dtype, *shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (scale * torch.randn(*shape, device=DEV, generator=g)).to(dtype)


def exact(dtype):                      # tolerance of the existing tests for results that are one rounding of an fp32 value
    return 1e-6 if dtype == F32 else 1e-2


# case -> the dtypes in which no other GPU test launches its entry points (the table in the module docstring)
GAPS = {
    "gelu": [H],
    "dropout": [H],
    "add_rowvec_mask": [H],
    "embedding_fwd_scalar": [F32, BF, H],
    "gather_rows": [F32, H],
    "gather_scatter_parts": [F32, H],
    "segment_rowsum": [H],
    "colsum": [F32, H],
    "mul": [F32, H],
    "scale_row_groups": [H],
    "cross_entropy": [H],
    "probs": [F32, BF, H],
    "adam": [F32],
    "bias_block": [F32, H],
    "bias_outer_grad": [F32, H],
    "bias_build": [H],
    "mean_heads": [F32, H],
    "c_attn_grad": [H],
    "maxpool_relu": [H],
    "sync_batchnorm": [H],
    "join": [H],
    "attn_softmax": [H],
    "attn_decode": [H],
    "im2col_nchw": [H],
}


def cells(name):
    return pytest.mark.parametrize("dtype", GAPS.get(name, []), ids=lambda d: str(d).replace("torch.", ""))


@cells("gelu")
def test_gelu_fwd_bwd(K, dtype):
    x, dy = rnd(dtype, 5, cols_of(dtype)), rnd(dtype, 5, cols_of(dtype), seed=1)
    xr = x.float().requires_grad_(True)
    yr = F.gelu(xr)
    yr.backward(dy.float())
    assert rel(K.gelu_fwd(x), yr.detach()) < tol(dtype) and rel(K.gelu_bwd(dy, x), xr.grad) < tol(dtype)


@cells("dropout")
def test_dropout_add_and_bwd(K, dtype):
    x, res, dy = (rnd(dtype, 5, cols_of(dtype), seed=s) for s in range(3))
    kept = K.dropout_add(torch.ones_like(x), None, 0.1, 1234, 77).float() > 0
    want = torch.where(kept, x.float() / 0.9, torch.zeros_like(x.float())) + res.float()
    assert rel(K.dropout_add(x, res, 0.1, 1234, 77), want) < (1e-6 if dtype == F32 else 2e-2)
    assert rel(K.dropout_bwd(dy, 0.1, 1234, 77), torch.where(kept, dy.float() / 0.9, torch.zeros_like(dy.float()))) < exact(dtype)
    assert rel(K.dropout_add(x, res, 0.0, 1, 0), x.float() + res.float()) < tol(dtype)


@cells("add_rowvec_mask")
def test_add_rowvec_mask(K, dtype):
    c = cols_of(dtype)
    x, res, vec = rnd(dtype, 5, c), rnd(dtype, 5, c, seed=1), rnd(dtype, c, seed=2)
    mask = torch.tensor([False, True, False, False, True], device=DEV)
    ref = (x.float() + res.float() + vec.float()) * (~mask).float()[:, None]
    assert rel(K.add_rowvec_mask(x, res, vec, mask), ref) < tol(dtype)


@cells("embedding_fwd_scalar")
def test_embedding_fwd_odd_width(K, dtype):
    """A width that is no whole number of 16-byte vectors: the scalar kernel (the vector kernel runs in test_embedding / test_fp16_gpu)."""
    w = rnd(dtype, 11, cols_of(dtype) + 1)
    ids = torch.tensor([[3, 1, 10], [0, 1, 7], [1, 9, 9]], device=DEV)
    assert torch.equal(K.embedding_fwd(w, ids), w[ids])


@cells("gather_rows")
def test_gather_rows(K, dtype):
    src = rnd(dtype, 7, cols_of(dtype))
    idx = torch.tensor([6, -1, 0, 3, 3], device=DEV)
    want = torch.where((idx >= 0)[:, None], src[idx.clamp_min(0)], torch.zeros_like(src[:1]))
    assert torch.equal(K.gather_rows(src, idx), want)


@cells("gather_scatter_parts")
def test_gather_rows_parts_and_scatter_rows_part(K, dtype):
    D, B = cols_of(dtype), 2
    parts = [rnd(dtype, B, n, D, seed=n) for n in (3, 2)]
    cat = torch.cat(parts, 1).reshape(-1, D)                 # row b * 5 + t
    idx = torch.tensor([9, 0, 4, 7], device=DEV)
    packed = K.gather_rows_parts(parts, idx)
    assert torch.equal(packed, cat[idx])
    inverse = torch.full((B * 5,), -1, dtype=torch.int64, device=DEV)
    inverse[idx] = torch.arange(4, device=DEV)
    got = K.scatter_rows_part(packed, inverse, B, 2, 5, 3)    # the second part: positions 3, 4 of every sample
    want = torch.zeros(B * 5, D, device=DEV, dtype=dtype)
    want[idx] = packed
    assert torch.equal(got, want.view(B, 5, D)[:, 3:5])


@cells("colsum")
def test_colsum(K, dtype):
    x = rnd(dtype, 5, cols_of(dtype))
    base = rnd(dtype, cols_of(dtype), seed=1)
    assert rel(K.colsum(x, alpha=0.5), 0.5 * x.float().sum(0)) < 1e-5            # fp32 output
    got = K.colsum(x, alpha=0.5, out=base.clone(), accumulate=True)                # output in the operand's type
    assert got.dtype == dtype and rel(got, base.float() + 0.5 * x.float().sum(0)) < exact(dtype)


@cells("mul")
def test_mul_and_mul_rowvec(K, dtype):
    c = cols_of(dtype)
    a, b, v = rnd(dtype, 5, c), rnd(dtype, 5, c, seed=1), rnd(dtype, c, seed=2)
    assert rel(K.mul(a, b), a.float() * b.float()) < exact(dtype) and rel(K.mul_rowvec(a, v), a.float() * v.float()) < exact(dtype)


@cells("scale_row_groups")
def test_scale_row_groups(K, dtype):
    x = rnd(dtype, 4, cols_of(dtype))
    s = torch.tensor([0.5, -2.0], device=DEV)
    assert rel(K.scale_row_groups(x, s, 2), x.float() * s.repeat_interleave(2)[:, None]) < exact(dtype)


@cells("cross_entropy")
def test_cross_entropy_fwd_bwd(K, dtype):
    V = cols_of(dtype) - 3                                    # a padded row: ld = V + 3
    store = rnd(dtype, 5, V + 3, scale=3.0)
    target = torch.tensor([0, 1, V - 1, 7, 1], device=DEV)
    lr = store[:, :V].float().requires_grad_(True)
    loss = F.nll_loss(F.log_softmax(lr, -1), target, ignore_index=1, reduction="sum")
    loss.backward()
    lse, row_loss = K.cross_entropy_fwd(store, target, V, 1)
    assert rel(row_loss.sum(), loss.detach()) < 1e-5
    d = K.cross_entropy_bwd(store, target, lse, torch.tensor([1.0], device=DEV), V, 1)
    assert rel(d[:, :V], lr.grad) < (1e-5 if dtype == F32 else 1e-2) and float(d[:, V:].float().abs().max()) == 0.0


@cells("probs")
def test_probs_fwd_bwd(K, dtype):
    V = cols_of(dtype) - 3                                    # (probs_bwd pads its rows to a multiple of 8: 24 / 40 columns)
    store = rnd(dtype, 5, V + 3, scale=2.0)
    lr = store[:, :V].float().requires_grad_(True)
    for log_probs in (False, True):
        lr.grad = None
        yr = F.log_softmax(lr, -1) if log_probs else F.softmax(lr, -1)
        dy = rnd(F32, 5, V, seed=3)
        yr.backward(dy)
        y = K.probs_fwd(store, V, V + 3, log_probs)
        assert rel(y, yr.detach()) < 1e-5
        assert rel(K.probs_bwd(dy, y, V, dtype, log_probs)[:, :V], lr.grad) < (1e-5 if dtype == F32 else 1e-2)


@cells("adam")
def test_adam_step(K, dtype):
    n = 5 * cols_of(dtype) + 3
    p0, g = rnd(F32, n), rnd(dtype, n, seed=1)
    master, m, v, model = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), p0.clone().to(dtype)
    K.adam_step(master, m, v, g, model, None, 1e-2, 0.9, 0.98, 1e-8, 0.01, 1)
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pr], lr=1e-2, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01)
    pr.grad = g.float()
    opt.step()
    assert rel(master, pr.detach()) < 1e-5 and torch.equal(model, master.to(dtype))


@cells("bias_block")
def test_bias_block_add_slice_grad(K, dtype):
    B, A, T, n, s = 2, 3, 7, 3, 2
    bias, vals, vb = rnd(dtype, B, A, T, T), rnd(dtype, n, n, A, seed=1), rnd(dtype, B, A, n, n, seed=2)
    ref = bias.float().clone()
    ref[:, :, s:s + n, s:s + n] += vals.float().permute(2, 0, 1)
    assert rel(K.bias_block_add_(bias.clone(), vals, s), ref) < exact(dtype)
    ref = bias.float().clone()
    ref[:, :, s:s + n, s:s + n] += vb.float()
    assert rel(K.bias_block_add_batch_(bias.clone(), vb, s), ref) < exact(dtype)
    assert torch.equal(K.bias_block_slice(bias, s, n), bias[:, :, s:s + n, s:s + n])
    assert rel(K.bias_block_grad(bias, s, n), bias.float()[:, :, s:s + n, s:s + n].sum(0).permute(1, 2, 0)) < exact(dtype)


@cells("mean_heads")
def test_mean_heads(K, dtype):
    p = rnd(dtype, 2 * 3, 5, 7)
    assert rel(K.mean_heads(p, 2, 3), p.float().view(2, 3, 5, 7).mean(1)) < exact(dtype)


@cells("c_attn_grad")
def test_c_attn_grad(K, dtype):
    B, Hd, T, ld = 3, 4, 5, 8
    delta = rnd(F32, B * Hd, ld)
    c = (torch.rand(Hd, device=DEV) + 0.5).to(dtype)
    want = delta.view(B, Hd, ld)[:, :, :T].double().sum(dim=(0, 2)) / c.double()
    got = K.c_attn_grad(delta, c, B, Hd, T)
    assert got.dtype == dtype and rel(got.float(), want.float()) < (1e-5 if dtype == F32 else 8e-3)


@cells("maxpool_relu")
def test_maxpool_and_relu(K, dtype):
    B, C, Hh, Ww = 1, cols_of(dtype), 5, 3
    x = rnd(dtype, B, C, Hh, Ww)
    rows = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    xr = x.float().requires_grad_(True)
    ref = F.max_pool2d(xr, 3, 2, 1)
    dy = rnd(dtype, *ref.shape, seed=1)
    ref.backward(dy.float())
    y, arg, _, _ = K.maxpool_fwd(rows, B, Hh, Ww, C, 3, 2, 1)
    assert torch.equal(y.float(), ref.permute(0, 2, 3, 1).reshape(-1, C))
    dx = K.maxpool_bwd(dy.permute(0, 2, 3, 1).reshape(-1, C).contiguous(), arg, B, Hh, Ww, C, 3, 2, 1)
    assert rel(dx, xr.grad.permute(0, 2, 3, 1).reshape(-1, C)) < exact(dtype)
    assert torch.equal(K.relu(rows), F.relu(rows)) and torch.equal(K.relu(rows, gate=rows), rows * (rows > 0))


@cells("segment_rowsum")
def test_segment_rowsum(K, dtype):
    from ofasys_amd import ops
    V, D = 9, 12
    ids = torch.tensor([[3, 1, 8], [0, 1, 3], [3, 8, 8]], device=DEV)
    dout = rnd(dtype, 9, D)
    plan = ops.SegmentPlan.get((("dtype_dispatch", str(dtype)), tuple(ids.shape), str(ids.device)), ids)
    acc = torch.ones(V, D, device=DEV, dtype=dtype)
    K.segment_rowsum(dout, plan, acc, True)
    want = torch.zeros(V, D, device=DEV).index_add_(0, ids.reshape(-1), dout.float())
    assert rel(acc.float(), want + 1.0) < (1e-5 if dtype == F32 else 2e-2)


@cells("bias_outer_grad")
def test_bias_outer_grad(K, dtype):
    """Both forms: 16-byte pieces (start, T and P multiples of 4) and element-wise."""
    A = 3
    for Fr, P, s0, Tt in ((2, 4, 4, 16), (2, 3, 1, 9)):
        G = rnd(dtype, 1, A, Tt, Tt, seed=P)
        dvf, dvi = K.bias_outer_grad(G, s0, Fr, P)
        blk = G[0, :, s0:s0 + Fr * P, s0:s0 + Fr * P].float().view(A, Fr, P, Fr, P)
        assert rel(dvf, blk.sum((2, 4)).permute(1, 2, 0)) < 4e-3 and rel(dvi, blk.sum((1, 3)).permute(1, 2, 0)) < 4e-3


@cells("bias_build")
def test_bias_build_row_major_result(K, dtype):
    A, T, s, n = 3, 40, 5, 20
    abs_b, v = rnd(dtype, A, T, T), rnd(dtype, n, n, A, seed=1)
    out, _ = K.bias_build(abs_b, [s], [v])
    ref = abs_b.clone()
    ref[:, s:s + n, s:s + n] += v.permute(2, 0, 1)
    assert torch.equal(out, ref)


@cells("sync_batchnorm")
def test_sync_batchnorm_phases_on_one_rank(K, dtype):
    """ofa_batchnorm_fwd_stats / _fwd_apply / _bwd_stats / _bwd_dx chained without an exchange == BatchNorm over the rows."""
    rows, C = 5, cols_of(dtype)
    x, dy = rnd(dtype, rows, C, scale=1.5), rnd(dtype, rows, C, seed=1)
    w, b = (torch.rand(C, device=DEV) + 0.5).to(dtype), rnd(dtype, C, seed=2, scale=0.1)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    sums = K.batchnorm_fwd_stats(x)
    y, mean, rstd = K.batchnorm_fwd_apply(x, w, b, rm, rv, sums, 0.1, 1e-3)
    bsums, dw, db = K.batchnorm_bwd_stats(dy, y, x, w, mean, rstd, False)
    dx, _ = K.batchnorm_bwd_dx(dy, y, x, w, mean, rstd, bsums, sums[2 * C:], False)
    xr, wr, br = (t.float().requires_grad_(True) for t in (x, w, b))
    yr = F.batch_norm(xr, None, None, wr, br, True, 0.1, 1e-3)
    yr.backward(dy.float())
    t = 1.6e-2
    assert rel(y, yr) < t and rel(dx, xr.grad) < t and rel(dw, wr.grad) < 2 * t and rel(db, br.grad) < 2 * t


@cells("join")
@pytest.mark.parametrize("cols", [40, 256])
def test_residual_join_fwd_bwd(K, dtype, cols):
    """y = res + LN_a(x), z = LN_b(y) without dropout, and the gradients of x and res from (dy, dz): the split-row kernels (40 columns)
    and the 16-bit row-per-wave kernels (256)."""
    from ofasys_amd import ops
    rows = 5
    x, r, dy, dz = (rnd(dtype, rows, cols, seed=i) for i in range(4))
    lna, lnb = (torch.nn.LayerNorm(cols).to(DEV).to(dtype) for _ in range(2))
    with torch.no_grad():
        for i, ln in enumerate((lna, lnb)):
            ln.weight.copy_(1 + 0.1 * rnd(F32, cols, seed=10 + i)); ln.bias.copy_(0.1 * rnd(F32, cols, seed=20 + i))
    xx, rr = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    ops.manual_seed(99)
    y, z = ops.residual_join(xx, rr, lna, 0.0, True, lnb)
    torch.autograd.backward([y, z], [dy, dz])
    xf, rf = x.float().requires_grad_(True), r.float().requires_grad_(True)
    yf = rf + F.layer_norm(xf, (cols,), lna.weight.float(), lna.bias.float(), lna.eps)
    zf = F.layer_norm(yf, (cols,), lnb.weight.float(), lnb.bias.float(), lnb.eps)
    torch.autograd.backward([yf, zf], [dy.float(), dz.float()])
    for got, want in ((y, yf), (z, zf), (xx.grad, xf.grad), (rr.grad, rf.grad)):
        assert rel(got, want.detach()) < tol(dtype)


@cells("attn_softmax")
def test_attn_softmax(K, dtype):
    B, A, T, S = 2, 3, 5, 21
    x, bias = rnd(dtype, B * A, T, S), rnd(dtype, B * A, T, S, seed=1)
    kpm = torch.zeros(B, S, dtype=torch.bool, device=DEV)
    kpm[1, 15:] = True
    w = (x.float() * 0.3 + bias.float()).view(B, A, T, S).masked_fill(kpm[:, None, None, :], float("-inf")).view(B * A, T, S)
    assert rel(K.attn_softmax(x, bias, kpm, 0.3, A, False), torch.softmax(w, -1)) < exact(dtype)


@cells("attn_decode")
def test_attn_decode(K, dtype):
    B, Hd, S, cap = 2, 3, 7, 16
    D = Hd * 64
    q, kc, vc = rnd(dtype, B, D), rnd(dtype, B, cap, D, seed=1), rnd(dtype, B, cap, D, seed=2)
    bias = rnd(dtype, B * Hd, S, seed=3)
    c = (torch.rand(Hd, device=DEV) + 0.5).to(dtype)
    out, probs = K.attn_decode(q, kc, vc, S, Hd, 0.0884, bias=bias, c_attn=c, need_probs=True)
    kf = kc[:, :S].float().view(B, S, Hd, 64).transpose(1, 2)
    vf = vc[:, :S].float().view(B, S, Hd, 64).transpose(1, 2)
    p = torch.softmax((q.float().view(B, Hd, 1, 64) @ kf.transpose(2, 3)) * 0.0884 + bias.float().view(B, Hd, 1, S), dim=-1)
    o = (p @ vf) * c.float().view(1, Hd, 1, 1)
    assert rel(out.float(), o.transpose(1, 2).reshape(B, D)) < 1.5e-2 and rel(probs.float(), p.reshape(B * Hd, S)) < 1.5e-2


@cells("im2col_nchw")
@pytest.mark.parametrize("k,stride,pad,hw", [(3, 2, 1, 7), (12, 1, 0, 13)])
def test_im2col_from_the_nchw_image(K, dtype, k, stride, pad, hw):
    """The stem convolution's gather straight from the [B, C, H, W] image: rows staged in LDS (k = 3) and, for a row of more than
    48 KB / 64 (k = 12), the generic kernel; taps ordered (kh, kw, c), bit for bit against unfold."""
    B, C = 2, 3
    img = rnd(dtype, B, C, hw, hw)
    col, Ho, Wo = K.im2col(img, B, hw, hw, C, k, k, stride, pad, nchw=True)
    ref = F.unfold(img.float(), k, padding=pad, stride=stride).view(B, C, k, k, Ho * Wo).permute(0, 4, 2, 3, 1).reshape(B * Ho * Wo, -1)
    assert torch.equal(col[:, :C * k * k].float(), ref)
