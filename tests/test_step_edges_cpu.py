"""CPU: the step-edge entry points validate their arguments before any launch and report OFA_ERR_* through the status code."""
import pytest

from ofasys_amd import lib as L


def test_step_edge_exports_return_status_codes():
    h = L.lib()
    # id-major token gradient: NULL buffers, an id list beyond the LDS budget, rows that are no whole 16-byte vectors
    with pytest.raises(L.OfaError, match=r"status 1.*embedding_bwd_ids"):
        h.call("ofa_embedding_bwd_ids", None, None, None, 4, 768, 300, -1, 1, L.BF16, None)
    with pytest.raises(L.OfaError, match=r"status 2.*embedding_bwd_ids"):
        h.call("ofa_embedding_bwd_ids", 16, 16, 16, 1 << 20, 768, 51265, -1, 1, L.BF16, None)
    with pytest.raises(L.OfaError, match=r"status 2.*embedding_bwd_ids"):
        h.call("ofa_embedding_bwd_ids", 16, 16, 16, 4, 12, 300, -1, 1, L.BF16, None)
    with pytest.raises(L.OfaError, match=r"status 2.*aligned"):
        h.call("ofa_embedding_bwd_ids", 8, 16, 16, 4, 768, 300, -1, 1, L.BF16, None)
    with pytest.raises(L.OfaError, match=r"status 1.*embedding_bwd_ids"):
        h.call("ofa_embedding_bwd_ids", 16, 16, 16, 4, 768, 300, -1, 0, L.BF16, None)               # slices < 1
    with pytest.raises(L.OfaError, match="dtype"):
        h.call("ofa_embedding_bwd_ids", 16, 16, 16, 4, 768, 300, -1, 1, 7, None)
    h.call("ofa_embedding_bwd_ids", 16, 16, 16, 0, 768, 300, -1, 1, L.BF16, None)                    # nothing to do: no launch
    assert h.cdll.ofa_embedding_bwd_ids_ok(8192, 768, 51265, L.BF16) == 1
    assert h.cdll.ofa_embedding_bwd_ids_ok(1 << 20, 768, 51265, L.BF16) == 0
    assert h.cdll.ofa_embedding_bwd_ids_ok(100, 4, 300, L.BF16) == 0 and h.cdll.ofa_embedding_bwd_ids_ok(100, 4, 300, L.F32) == 1
    # range lookup: rows beyond the table, a negative start, unvectorizable rows
    with pytest.raises(L.OfaError, match=r"status 1.*embedding_range_bwd"):
        h.call("ofa_embedding_range_bwd", 16, 16, 2, 8, 768, 10, 3, L.BF16, None)                    # rows 3 .. 11 of 10
    with pytest.raises(L.OfaError, match=r"status 1.*embedding_range_bwd"):
        h.call("ofa_embedding_range_bwd", 16, 16, 2, 5, 768, 10, -1, L.BF16, None)
    with pytest.raises(L.OfaError, match=r"status 1.*embedding_range_bwd"):
        h.call("ofa_embedding_range_bwd", 16, 16, 0, 5, 768, 10, 0, L.BF16, None)                    # batch < 1
    with pytest.raises(L.OfaError, match=r"status 2.*embedding_range_bwd"):
        h.call("ofa_embedding_range_bwd", 16, 16, 2, 5, 12, 10, 0, L.BF16, None)
    h.call("ofa_embedding_range_bwd", 16, 16, 2, 0, 768, 10, 0, L.BF16, None)                        # T == 0: no launch
    # the product library has one path whatever the environment says
    assert [h.cdll.ofa_step_edges_old(i) for i in range(4)] == [0, 0, 0, 0]
    with pytest.raises(L.OfaError, match="im2col_patch"):
        h.call("ofa_im2col_patch", 16, 16, 2, 3, 28, 28, 14, 500, 0, L.BF16, None)                   # Kpad < C * p * p


def test_debug_library_honours_the_old_path_mask(monkeypatch):
    """libofasys_amd_dbg.so: OFA_STEP_EDGES_OLD is a bit mask over the OFA_EDGE_* items (read at every call)."""
    import ctypes
    import os
    dbg = os.path.join(os.path.dirname(L.LIB_PATH), "libofasys_amd_dbg.so")
    assert os.path.exists(dbg), "build with `python __graft_entry__.py` first"
    fn = ctypes.CDLL(dbg).ofa_step_edges_old
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int]
    monkeypatch.delenv("OFA_STEP_EDGES_OLD", raising=False)
    assert [fn(i) for i in range(4)] == [0, 0, 0, 0]
    monkeypatch.setenv("OFA_STEP_EDGES_OLD", "10")                       # token table + im2col
    assert [fn(i) for i in range(4)] == [0, 1, 0, 1]
    monkeypatch.setenv("OFA_STEP_EDGES_OLD", "15")
    assert [fn(i) for i in range(4)] == [1, 1, 1, 1]
    assert [L.lib().cdll.ofa_step_edges_old(i) for i in range(4)] == [0, 0, 0, 0] or "dbg" in L.LIB_PATH
