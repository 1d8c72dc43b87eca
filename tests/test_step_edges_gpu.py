"""The one-launch forms at the edges of the train step (token-table gradient id-major, position tables looked up by arange, im2col in
dword runs) against the paths they replace, bit for bit on the same inputs.  The output gradients are pre-filled with random values:
these kernels accumulate."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ofasys_amd import kernels
    return kernels


def _token_ids(n, V, pad):
    """n ids below V: id 7 more than 64 times (spread over the list), id 3 only at position 0, id 5 only at n - 1, the padding id, one id
    out of range on each side; everything else drawn from 10 .. V - 1 (so ids below 10 other than these never occur)."""
    g = torch.Generator().manual_seed(n * 131 + V)
    ids = torch.randint(10, V, (n,), generator=g)
    if n >= 8:
        heavy = torch.randperm(n - 2, generator=g)[:min(n // 2, 70)] + 1
        ids[heavy] = 7
        free = [i for i in range(1, n - 1) if ids[i] != 7]
        ids[free[0]] = pad
        ids[free[1]] = V + 5
        ids[free[2]] = -2
        ids[free[3]] = pad
    ids[0] = 3
    ids[n - 1] = 5 if n > 1 else 3
    return ids


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,V,D", [(130, 300, 768), (130, 300, 8), (130, 5000, 768), (1, 5000, 768), (1, 300, 8), (2100, 5000, 768), (2100, 300, 768)])
def test_token_backward_id_major_equals_row_major(K, n, V, D, dtype):
    """ofa_embedding_bwd_ids against ofa_embedding_bwd as kernels.embedding_bwd calls it (V = 300: sliced partial sums; V = 5000: the
    presence-buffer branch, one slice): equal bits, rows of absent ids untouched.  n = 130 is no multiple of the 64-id ballot; n = 2100
    gives a wave several positions and, at V = 300, owners whose rows lie in several slices."""
    pad = 1
    ids = _token_ids(n, V, pad).to(DEV)
    torch.manual_seed(n + D)
    dout = torch.randn(n, D, device=DEV).to(dtype)
    fill = torch.randn(V, D, device=DEV).to(dtype)
    old = K.embedding_bwd(dout, ids, V, pad, dweight=fill.clone(), id_major=False)
    new = K.embedding_bwd(dout, ids, V, pad, dweight=fill.clone(), id_major=True)
    assert torch.equal(new.view(torch.uint8), old.view(torch.uint8))
    present = torch.zeros(V, dtype=torch.bool, device=DEV)
    ok = (ids >= 0) & (ids < V) & (ids != pad)
    present[ids[ok]] = True
    assert torch.equal(new[~present].view(torch.uint8), fill[~present].view(torch.uint8))          # absent ids, the padding row
    assert not torch.equal(new[present], fill[present])
    # and against a plain fp32 index_add, to rounding: the two agree on the RIGHT sum
    ref = fill.float().index_add(0, ids[ok], dout[ok].float())
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert float((new.float() - ref).abs().max()) <= tol * float(ref.abs().max())


def test_token_backward_auto_route(K):
    """kernels.embedding_bwd by itself: id-major for a one-slice (wide-vocabulary) table, row-major when the id list exceeds the LDS
    budget or the table is sliced -- the same bits whichever it takes."""
    from ofasys_amd.lib import lib
    assert lib().cdll.ofa_embedding_bwd_ids_ok(15360, 768, 51265, 1) == 1
    assert lib().cdll.ofa_embedding_bwd_ids_ok(15361, 768, 51265, 1) == 0          # beyond the LDS budget
    assert lib().cdll.ofa_embedding_bwd_ids_ok(100, 12, 51265, 1) == 0             # rows that are no whole 16-byte vectors
    V, D, pad = 60000, 64, 1                                                       # one slice: kernels.embedding_bwd goes id-major by itself
    assert lib().cdll.ofa_embedding_bwd_slices(V, D) == 1
    ids = _token_ids(500, V, pad).to(DEV)
    dout = torch.randn(500, D, device=DEV).bfloat16()
    fill = torch.randn(V, D, device=DEV).bfloat16()
    auto = K.embedding_bwd(dout, ids, V, pad, dweight=fill.clone())
    old = K.embedding_bwd(dout, ids, V, pad, dweight=fill.clone(), id_major=False)
    assert torch.equal(auto.view(torch.uint8), old.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("T", [5, 10])
def test_position_range_backward_equals_batch_sum_and_scatter(K, T, B, dtype):
    """ofa_embedding_range_bwd on a 10-row table against ofa_batch_sum + ofa_embedding_bwd with ids = arange(T): equal bits, rows >= T
    untouched; and from a row offset."""
    V, D = 10, 768
    torch.manual_seed(T * 10 + B)
    g = torch.randn(B, T, D, device=DEV).to(dtype)
    fill = torch.randn(V, D, device=DEV).to(dtype)
    ids = torch.arange(T, device=DEV).unsqueeze(0)
    db = K.batch_sum(g, B).view(1, T, D) if B > 1 else g
    old = K.embedding_bwd(db, ids, V, -1, dweight=fill.clone(), id_major=False)
    new = K.embedding_range_bwd(g, fill.clone(), 0, T)
    assert torch.equal(new.view(torch.uint8), old.view(torch.uint8))
    assert torch.equal(new[T:].view(torch.uint8), fill[T:].view(torch.uint8))
    assert not torch.equal(new[:T], fill[:T])
    if T == 5:
        old = K.embedding_bwd(db, ids + 3, V, -1, dweight=fill.clone(), id_major=False)
        new = K.embedding_range_bwd(g, fill.clone(), 3, T)
        assert torch.equal(new.view(torch.uint8), old.view(torch.uint8))
        assert torch.equal(new[:3].view(torch.uint8), fill[:3].view(torch.uint8)) and torch.equal(new[8:].view(torch.uint8), fill[8:].view(torch.uint8))


def _text_adaptor(dtype):
    from oracle.cases import CASES
    from tests.model_util import build_model
    case = dict(CASES["tiny_text"])
    case["overrides"] = {"use_self_attn_bias": False, "entangle_position_embedding": True}
    case["adaptor_overrides"] = {"text": {"entangle_position_embedding": True}}
    model, d = build_model(case, DEV, dtype)
    model.eval()                                     # dropout off: the two runs must see the same values
    return model.encoder.adaptor.text, d


@pytest.mark.parametrize("arena", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_text_adaptor_position_gradient_equals_generic_path(K, monkeypatch, dtype, arena):
    """TextAdaptor forward + backward (positions entangled into the embedding): the position table's gradient through the range route --
    fused into the add's backward when the table has an arena gradient, from EmbeddingFn.backward otherwise -- against batch sum + generic
    scatter-add on the same inputs; outputs and the other gradients equal too."""
    from ofasys_amd import ModalityType, Slot
    ad, d = _text_adaptor(dtype)
    B, T = 3, 9
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(4, len(d), (B, T), generator=g)
    tokens[1, 6:] = d.pad()
    tokens = tokens.to(DEV)
    w = ad.embed_positions.weight
    D = w.shape[1]
    dy = torch.randn(B, T, D, device=DEV, generator=torch.Generator(DEV).manual_seed(6)).to(dtype)
    fill = torch.randn(w.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(7)).to(dtype)
    launched = []
    real = K.embedding_range_bwd
    monkeypatch.setattr(K, "embedding_range_bwd", lambda *a: (launched.append(tuple(a[0].shape)), real(*a))[1])

    def run(old):
        monkeypatch.setattr(K, "edge_old", lambda item: bool(old))
        for p in ad.parameters():
            p.grad = None
        if arena:
            w._ofa_grad = fill.clone()
        try:
            out = ad(Slot(ModalityType.TEXT, True, tokens))
            out.embed.backward(dy)
            torch.cuda.synchronize()
            gpos = w._ofa_grad if arena else w.grad
            others = [p.grad.clone() for n, p in sorted(ad.named_parameters()) if p is not w and p.grad is not None]
            return out.embed.detach().clone(), gpos.clone(), others
        finally:
            if arena:
                del w._ofa_grad

    y_new, g_new, o_new = run(False)
    assert launched and launched[0][0] == (B * T if arena else T)        # the fused form read the [B * T, D] gradient / the plain one [T, D]
    n_launched = len(launched)
    y_old, g_old, o_old = run(True)
    assert len(launched) == n_launched                                   # the generic route never calls the range kernel
    assert torch.equal(y_new, y_old)
    assert torch.equal(g_new.view(torch.uint8), g_old.view(torch.uint8))
    if arena:
        assert torch.equal(g_new[T:].view(torch.uint8), fill[T:].view(torch.uint8))
    assert len(o_new) == len(o_old) and all(torch.equal(a, b) for a, b in zip(o_new, o_old))


def _unfold_reference(img, p, Kpad, lead):
    B, C, H, W = img.shape
    cols = F.unfold(img.float(), kernel_size=p, stride=p).transpose(1, 2)            # [B, N, C*p*p], N in (ph, pw) order, k = (c, i, j)
    N, Kc = cols.shape[1], cols.shape[2]
    ref = torch.zeros(B, lead + N, Kpad, device=img.device)
    ref[:, lead:, :Kc] = cols
    return ref.view(B * (lead + N), Kpad).to(img.dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("p,Kpad", [(14, 640), (14, 592), (7, 152), (2, 16)])
def test_im2col_patch_equals_unfold(K, p, Kpad, lead, dtype):
    """[2, 3, 28, 28] images: p = 14 moves dword runs (16-bit types), p = 7 and fp32 take the element-wise form; Kpad = 592 is the patch
    adaptor's own padding (588 -> 592: the last 16-byte store of a row is half data, half zeros), p = 2 puts four runs into one store.
    The output buffer is pre-filled: the zero columns and lead rows are written, not assumed."""
    torch.manual_seed(p)
    from ofasys_amd.lib import dtype_code, lib, ptr, stream
    img = torch.randn(2, 3, 28, 28, device=DEV).to(dtype)
    ref = _unfold_reference(img, p, Kpad, lead)
    col = torch.full(ref.shape, 7.0, device=DEV, dtype=dtype)
    lib().call("ofa_im2col_patch", ptr(img), ptr(col), 2, 3, 28, 28, p, Kpad, lead, dtype_code(img), stream())
    assert torch.equal(col, ref)
    assert torch.equal(K.im2col_patch(img, p, Kpad, lead), ref)
    # an image view at an odd element offset is not dword-aligned: the element-wise form, the same matrix
    buf = torch.zeros(img.numel() + 1, device=DEV, dtype=dtype)
    buf[1:] = img.reshape(-1)
    assert torch.equal(K.im2col_patch(buf[1:].view(img.shape), p, Kpad, lead), ref)


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("cols", [768, 8])
@pytest.mark.parametrize("rows", [1, 63, 1000, 1100, 5000])
def test_queued_column_sums_equal_immediate_ones(K, rows, cols, out_dtype):
    """kernels.colsum(fold=queue, same_bits=True) -- the adaptors' type-vector / patch-bias / class-token gradients in the batched fold
    launch -- against the immediate final pass on the same inputs, bit for bit: up to 1024 rows (at most 16 row groups) either order is
    the slot order; 1100 and 5000 rows (18 and 79 groups) need the queue's sixteen-lane order.  Two jobs to different outputs share a
    flush; a second contribution to one output is kept out of the first one's launch and lands after it."""
    torch.manual_seed(rows + cols)
    x1 = torch.randn(rows, cols, device=DEV).bfloat16()
    x2 = torch.randn(rows, cols, device=DEV).bfloat16()
    fill1 = torch.randn(cols, device=DEV).to(out_dtype)
    fill2 = torch.randn(cols, device=DEV).to(out_dtype)
    want1 = K.colsum(x1, out=fill1.clone(), accumulate=True)
    want2 = K.colsum(x2, alpha=-1.0, out=fill2.clone(), accumulate=True)
    q = K.FoldQueue()
    got1, got2 = fill1.clone(), fill2.clone()
    K.colsum(x1, out=got1, accumulate=True, fold=q, same_bits=True)
    K.colsum(x2, alpha=-1.0, out=got2, accumulate=True, fold=q, same_bits=True)
    assert len(q.jobs) == 2 and torch.equal(got1, fill1)                  # both wait for the flush
    q.flush()
    assert torch.equal(got1.view(torch.uint8), want1.view(torch.uint8)) and torch.equal(got2.view(torch.uint8), want2.view(torch.uint8))
    # the same output twice (the patch-embedding bias: all rows, then minus the class-token rows)
    want = K.colsum(x2, alpha=-1.0, out=K.colsum(x1, out=fill1.clone(), accumulate=True), accumulate=True)
    got = fill1.clone()
    K.colsum(x1, out=got, accumulate=True, fold=q, same_bits=True)
    K.colsum(x2, alpha=-1.0, out=got, accumulate=True, fold=q, same_bits=True)
    assert len(q.jobs) == 1                                               # the first contribution went out in a launch of its own
    q.flush()
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    # and a strided view (the class-token rows of a [B, T, D] gradient)
    big = torch.randn(rows, 3, cols, device=DEV).bfloat16()
    want = K.colsum(big[:, 0, :], out=fill2.clone(), accumulate=True)
    got = fill2.clone()
    K.colsum(big[:, 0, :], out=got, accumulate=True, fold=q, same_bits=True)
    q.flush()
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
