"""CPU: the C-ABI library loads and exports every symbol include/ofasys_amd.h declares; no compute without a GPU."""
import ctypes
import os

import pytest
import torch

from ofasys_amd import lib as L


def test_header_parses_and_library_exports_every_symbol():
    protos = L.parse_header()
    assert len(protos) >= 40
    for must in ("ofa_gemm", "ofa_attn_fwd", "ofa_attn_bwd", "ofa_layernorm_fwd", "ofa_layernorm_bwd",
                 "ofa_scaled_softmax_fwd", "ofa_scaled_masked_softmax_fwd", "ofa_scaled_upper_triang_masked_softmax_fwd",
                 "ofa_scaled_softmax_bwd", "ofa_scaled_masked_softmax_bwd", "ofa_scaled_upper_triang_masked_softmax_bwd",
                 "ofa_get_batch_per_block", "ofa_embedding_bwd", "ofa_cross_entropy_fwd", "ofa_adam_step", "ofa_version",
                 "ofa_last_error", "ofa_im2col_patch", "ofa_bias_block_add", "ofa_batchnorm_route", "ofa_im2col_route"):
        assert must in protos
    assert os.path.exists(L.LIB_PATH), "build with `python __graft_entry__.py` first"
    cdll = ctypes.CDLL(L.LIB_PATH)
    for name in protos:
        getattr(cdll, name)          # AttributeError == declared but not exported
    h = L.lib()
    assert h.cdll.ofa_version() >= 100


def test_host_only_entry_points():
    h = L.lib()
    from oracle import restate
    for a in [(128, 128, 2, 4), (64, 448, 2, 4), (4, 16, 1, 1), (8, 4096, 1, 1), (16, 100, 3, 3)]:
        assert h.cdll.ofa_get_batch_per_block(*a) == restate.get_batch_per_block(*a)
    assert h.cdll.ofa_layernorm_bwd_ws_rows() > 0
    # the convolution stack's launch shapes (csrc/conv.hip; tests/test_conv_oracle_cpu.py checks them against every table entry)
    out = (ctypes.c_int * 3)()
    for rows, C, dt, want in [(25088, 512, L.BF16, (196, 5, 4096)), (32, 64, L.BF16, (1, 3, 1)), (32768 + 1, 64, L.F32, (256, 4, 2049)),
                              (1, 8, L.F16, (1, 0, 1))]:
        assert h.cdll.ofa_batchnorm_route(rows, C, dt, ctypes.addressof(out)) == 0 and tuple(out) == want, (rows, C, dt, tuple(out))
    assert h.cdll.ofa_batchnorm_route(4, 12, L.BF16, ctypes.addressof(out)) == 2 and h.cdll.ofa_batchnorm_route(4, 8, 7, ctypes.addressof(out)) == 1
    assert h.cdll.ofa_im2col_route(32, 192, 192, 3, 152, 1, L.BF16) == 2           # the image stem: 64 x 152 elements in LDS
    assert h.cdll.ofa_im2col_route(1, 5, 5, 8, 392, 1, L.BF16) == 0 and h.cdll.ofa_im2col_route(1, 5, 5, 6, 384, 1, L.F16) == 2    # 48 KB
    assert h.cdll.ofa_im2col_route(2, 7, 7, 64, 576, 0, L.BF16) == 1 and h.cdll.ofa_im2col_route(2, 7, 7, 3, 32, 0, L.BF16) == 0
    assert h.cdll.ofa_im2col_route(2, 7, 7, 4, 40, 0, L.F32) == 1 and h.cdll.ofa_im2col_route(2, 7, 7, 4, 40, 0, 9) == -1
    assert h.cdll.ofa_conv_out_size(384, 7, 2, 3) == 192 and h.cdll.ofa_conv_out_size(1, 2, 2, 0) == 0


def test_gemm_group_plan_is_host_only():
    """ofa_gemm_group_plan: one K-slice length for the group, at most 256 workgroups of 256 x 256 tiles in total."""
    import ctypes as C
    from ofasys_amd import kernels as K
    h = L.lib()

    def plan(shapes, dt=L.BF16):
        arr = (K._GroupItem * len(shapes))()
        for it, (m, n, k) in zip(arr, shapes):
            it.a, it.b, it.lda, it.ldb, it.m, it.n, it.k = 4096, 8192, m, n, m, n, k
        h.call("ofa_gemm_group_plan", C.addressof(arr), len(shapes), dt)
        return [it.splits for it in arr]

    assert plan([(768, 3072, 13312), (3072, 768, 13312), (2304, 768, 13312), (768, 768, 13312)]) == [2, 2, 2, 2]
    sp = plan([(2304, 768, 3072), (768, 768, 3072), (1536, 768, 13312), (768, 3072, 3072), (3072, 768, 3072)])
    tiles = [27, 9, 18, 36, 36]
    assert sum(t * s for t, s in zip(tiles, sp)) <= 256 and sp[2] > sp[0] >= 1        # the long contraction gets more slices
    assert plan([(256, 256, 64)]) == [1]
    assert plan([(4096, 4096, 1024), (4096, 4096, 512)]) == [1, 1]                     # more than one round already: no slicing
    assert plan([(768, 768, 100)]) == [1]                                              # any row count (round 4: zero rows inside the kernel)
    with pytest.raises(L.OfaError, match="gemm_group"):
        plan([(772, 768, 128)])                                                        # m % 8
    with pytest.raises(L.OfaError, match="gemm_group"):
        plan([(768, 768, 128)], L.F32)
    with pytest.raises(L.OfaError, match="gemm_group"):
        plan([(256, 256, 64)] * 17)
    # two base-size encoder layers in one group: a round of one-slice products (no slabs: ops._Wgrads.FLUSH_TILES)
    assert plan([(768, 3072, 13312), (3072, 768, 13312), (2304, 768, 13312), (768, 768, 13312)] * 2) == [1] * 8


def test_shipped_join_backward_is_the_row_per_wave_kernel():
    """Since round 6 the row-per-wave residual-join BACKWARD is the product's kernel (round 5 held it back for a fault that turned out to
    be the dK/dV attention kernel's: profiles/round6_graph_fault_root_cause.txt): 16-bit rows of 256 k columns hand one dropout keep bit
    per element from the forward to the backward, and the partial rows are sized for the row kernel; other shapes keep the split-row
    kernel and no keep bits."""
    h = L.lib()
    assert h.cdll.ofa_join_keep_bytes(13312, 768, L.BF16) == 13312 * 768 // 8 * 4 // 3 or h.cdll.ofa_join_keep_bytes(13312, 768, L.BF16) >= 13312 * 768 // 8
    assert h.cdll.ofa_join_keep_bytes(100, 1024, L.F16) >= 100 * 1024 // 8
    assert h.cdll.ofa_join_keep_bytes(100, 1000, L.BF16) == 0 and h.cdll.ofa_join_keep_bytes(100, 768, L.F32) == 0
    assert h.cdll.ofa_join_bwd_slots(13312, 768, L.BF16) == 256 and h.cdll.ofa_join_bwd_slots(60, 768, L.BF16) == 8     # 8 rows per block
    assert h.cdll.ofa_join_bwd_slots(60, 768, L.F32) == 20                                                               # split-row kernel


def test_status_codes_not_asserts():
    h = L.lib()
    # argument validation happens before any launch, so it is observable without a GPU
    with pytest.raises(L.OfaError, match="layernorm"):
        h.call("ofa_layernorm_fwd", None, None, None, None, None, None, 4, 6, 1e-5, L.BF16, None)   # cols % 8 != 0
    with pytest.raises(L.OfaError, match="sk"):
        h.call("ofa_scaled_softmax_fwd", 1, 1, 1.0, 1, 1, 4, 5000, L.F32, None)                       # sk > 4096
    with pytest.raises(L.OfaError, match="sk"):                                                        # same precondition, backward
        h.call("ofa_scaled_masked_softmax_bwd", 1, 1, 1, 1.0, 1, 1, 4, 5000, L.F16, None)
    with pytest.raises(L.OfaError, match="dtype"):
        h.call("ofa_scaled_upper_triang_masked_softmax_bwd", 1, 1, 1, 1.0, 1, 8, 7, None)
    with pytest.raises(L.OfaError, match="dtype"):                                                     # an unknown dtype code
        h.call("ofa_layernorm_fwd", 1, 1, 1, 1, 1, 1, 4, 8, 1e-5, 7, None)
    with pytest.raises(L.OfaError, match="bf16"):
        from ofasys_amd import kernels as K
        call = K._AttnCall(q=1, k=1, v=1, out=1, B=1, heads=1, T=32, S=32, Tpad=32, ldq=64, ldk=64, ldo=64, scale=1.0, dtype=L.F32)
        h.call("ofa_attn_fwd", ctypes.addressof(call), None)


def test_attn_call_mirrors_the_c_struct():
    """kernels._AttnCall is as large as the static_assert in csrc/attention.hip says ofa_attn_call is (no padding on either side)."""
    import re
    from ofasys_amd import kernels as K
    src = open(os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "attention.hip")).read()
    assert ctypes.sizeof(K._AttnCall) == int(re.search(r"static_assert\(sizeof\(ofa_attn_call\) == (\d+)", src).group(1)) == 280


def test_generation_descriptors_mirror_the_c_structs():
    """kernels._GenPolicy / _GenState are as large as the static_asserts in csrc/beam_search.hip say ofa_gen_policy / ofa_gen_state
    are, and carry the header's fields in the header's order."""
    import re
    from ofasys_amd import kernels as K
    src = open(os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "beam_search.hip")).read()
    header = re.sub(r"/\*.*?\*/", " ", open(L.HEADER).read(), flags=re.S)
    for mirror, name, size in ((K._GenPolicy, "ofa_gen_policy", 72), (K._GenState, "ofa_gen_state", 120)):
        assert ctypes.sizeof(mirror) == int(re.search(r"static_assert\(sizeof\(%s\) == (\d+)" % name, src).group(1)) == size
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        assert re.findall(r"(\w+)\s*[,;]", body) == [f[0] for f in mirror._fields_], name
    assert len(K._GenPolicy._fields_) == 14 and len(K._GenState._fields_) == 15


_P = 4096                     # a fake, 16-byte aligned device address: every descriptor below is refused before any launch
_SEG = dict(seg=_P, rows_q=64, rows_k=64)
_DSUM = dict(bias=_P, dbias=_P, ws=_P)
_ATTN_REFUSALS = [
    # (entry, shared bias, the one change to a valid-looking descriptor, the message of the check that refuses it)
    ("fwd", 0, dict(dtype=L.F32), r"status 2.*bf16 / fp16 only \(dtype 0\)"),
    ("bwd", 1, dict(dtype=7), r"status 2.*bf16 / fp16 only \(dtype 7\)"),
    ("fwd", 0, dict(heads=0), "bad shape B=2 heads=0 T=40 S=50"),
    ("bwd", 0, dict(S=-3), "bad shape B=2 heads=2 T=40 S=-3"),
    ("fwd", 0, dict(ldq=132), "leading dims must be multiples of 8"),
    ("bwd", 1, dict(ldo=129), "leading dims must be multiples of 8"),
    ("fwd", 0, dict(Tpad=32), r"Tpad must be a multiple of 32 covering T \(T=40 Tpad=32\)"),
    ("bwd", 0, dict(Tpad=72), r"Tpad must be a multiple of 32 covering T \(T=40 Tpad=72\)"),
    ("fwd", 0, dict(scale=0.0), "attn_fwd: the score scale must be positive .*got 0"),
    ("fwd", 1, dict(scale=-0.125), "attn_fwd: the score scale must be positive .*got -0.125"),
    ("fwd", 0, dict(v=None), "attn_fwd: null pointer"),
    ("fwd", 1, dict(lse=None), "attn_fwd: null pointer"),                  # (the dense forward takes lse == NULL)
    ("bwd", 0, dict(delta=None), "attn_bwd: null pointer"),
    ("bwd", 1, dict(out=None), "attn_bwd: null pointer"),                  # (the dense backward takes out == NULL: ofa_attn_bwd_prep)
    ("fwd", 0, dict(_SEG, bias=_P), r"attn_fwd: the ragged \(seg\) mode takes no"),
    ("bwd", 0, dict(_SEG, bias=_P), r"attn_bwd: the ragged \(seg\) mode takes no"),
    ("bwd", 0, dict(_SEG, dbias=_P), r"attn_bwd: the ragged \(seg\) mode takes no"),
    ("fwd", 0, dict(_SEG, kpm=_P), r"attn_fwd: the ragged \(seg\) mode takes no"),
    ("fwd", 1, dict(_SEG, kpm=_P), r"attn_fwd: the ragged \(seg\) mode takes no"),
    ("bwd", 0, dict(_SEG, kpm=_P), r"attn_bwd: the ragged \(seg\) mode takes no"),
    ("bwd", 1, dict(_SEG, kpm=_P), r"attn_bwd: the ragged \(seg\) mode takes no"),
    ("fwd", 0, dict(_SEG, lse=None), r"attn_fwd: the ragged \(seg\) mode .* needs lse"),
    ("fwd", 0, dict(_SEG, seg=_P + 4), r"attn_fwd: the ragged \(seg\) mode .* 16-byte aligned table"),
    ("bwd", 1, dict(_SEG, seg=_P + 8), r"attn_bwd: the ragged \(seg\) mode .* 16-byte aligned table"),
    ("fwd", 0, dict(_SEG, rows_q=0), "attn_fwd: ragged mode needs rows_q / rows_k"),
    ("bwd", 1, dict(_SEG, rows_k=0), "attn_bwd: ragged mode needs rows_q / rows_k"),
    ("bwd", 0, dict(_SEG, rows_q=96), "attn_bwd: ragged mode needs rows_q / rows_k and Tpad >= rows_q"),
    ("fwd", 1, dict(Tb=0), r"attn_fwd: the swizzled bias image is of \[heads, Tb, Sb\] \(Tb=0 Sb=60\)"),
    ("fwd", 1, dict(bias_swz_row=_P + 8), "attn_fwd: the swizzled bias image must be 16-byte aligned"),
    ("fwd", 1, dict(Tb=39), "attn_fwd: the shared bias covers 39 x 60 positions, the call needs 40 x 50"),
    ("bwd", 1, dict(Sb=49), "attn_bwd: the shared bias covers 48 x 49 positions, the call needs 40 x 50"),
    ("bwd", 1, dict(bias_swz_col=None), "attn_bwd: the column image of the shared bias"),
    ("bwd", 1, dict(bias_swz_col=_P + 4), "attn_bwd: the column image of the shared bias"),
    ("bwd", 1, dict(dbias=_P), "attn_bwd: the column image of the shared bias .* for dbias, the row-major tensor"),
    ("fwd", 0, dict(c_attn_dtype=7), "attn_fwd: bad c_attn dtype 7"),
    ("bwd", 1, dict(c_attn_dtype=3), "attn_bwd: bad c_attn dtype 3"),
    ("bwd", 0, dict(cs_q=_P, cs_ldq=120), r"heads \* 64 = 128 floats \(row strides 120 / 0\)"),
    ("bwd", 1, dict(cs_v=_P, cs_ldq=128, cs_ldk=127), r"heads \* 64 = 128 floats \(row strides 128 / 127\)"),
    ("bwd", 0, dict(cs_c=_P), "attn_bwd: cs_c .* without c_attn"),
    ("bwd", 1, dict(_DSUM, dbias_dtype=5), "attn_bwd: bad dbias dtype 5"),
    # 2 heads x one [128 x 64] tile: the 2 samples become 2 chunks of 2 * 48 * 60 floats each
    ("bwd", 1, dict(_DSUM, ws_bytes=46079), "attn_bwd: the batch-sum kernel needs 46080 bytes of workspace for 2 chunks"),
    ("bwd", 1, dict(_DSUM, ws=None, ws_bytes=46080), "attn_bwd: the batch-sum kernel needs 46080 bytes of workspace for 2 chunks"),
    # 16 heads x 16 tiles fill the chip: one chunk of all 2049 samples, 16 bytes of LDS each on top of the 32 KiB of tiles
    ("bwd", 1, dict(_DSUM, B=2049, heads=16, ldq=1024, ldk=1024, ldo=1024, Tb=512, Sb=256), "status 2.*attn_bwd: 2049 samples per chunk exceed"),
]


@pytest.mark.parametrize("entry,shared,change,match", _ATTN_REFUSALS)
def test_attn_call_refusals(entry, shared, change, match):
    """Every precondition of ofa_attn_fwd / ofa_attn_bwd that is checked before the first launch, one changed field per row; the numbers
    in the messages come out of the descriptor, so they pin the field offsets of the ctypes mirror."""
    from ofasys_amd import kernels as K
    c = K._AttnCall(q=_P, k=_P, v=_P, out=_P, lse=_P, B=2, heads=2, T=40, S=50, Tpad=64, ldq=128, ldk=128, ldo=128, scale=0.125, dtype=L.BF16)
    if entry == "bwd":
        c.dout = c.delta = c.dq = c.dk = c.dv = _P
    if shared:
        c.bias_swz_row, c.Tb, c.Sb = _P, 48, 60
        if entry == "bwd":
            c.bias_swz_col = _P
    for name, value in change.items():
        setattr(c, name, value)
    with pytest.raises(L.OfaError, match=match):
        L.lib().call("ofa_attn_" + entry, ctypes.addressof(c), None)


def test_no_cpu_fallback():
    x = torch.randn(4, 8)
    with pytest.raises(L.OfaError, match="no CPU fallback"):
        L.ptr(x)
    from ofasys_amd import ops
    with pytest.raises(L.OfaError):
        ops.layer_norm(x, torch.ones(8), torch.zeros(8))
