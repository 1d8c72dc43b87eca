"""CPU: the host rule of first-touch gradient writes (ops.grad_begin / grad_mode / grad_end) alone, with fake sinks: a CPU tensor stands
for the gradient arena, the clearing launch is replaced by a recorder that fills the ranges with zeros, and a "sink" is a function
that asks ops.grad_mode for its view and then stores or adds as told."""
import pytest
import torch

from ofasys_amd import kernels as K
from ofasys_amd import ops


@pytest.fixture
def arena(monkeypatch):
    """A 64-element arena holding the sentinel 3.0 everywhere and the list of cleared ranges, one entry per clearing launch."""
    a = torch.full((64,), 3.0)
    launches = []

    def zero(ar, ranges, also=()):
        assert ar is a
        for t in also:
            t.zero_()
        launches.append(list(ranges))
        for lo, hi in ranges:
            ar[lo:hi] = 0

    monkeypatch.setattr(ops, "_zero_ranges", zero)
    yield a, launches
    ops.grad_abort()


def full_sink(view, value):
    """A full writer: every element of the view."""
    if ops.grad_mode(view, True):
        view += value
        return "add"
    view.fill_(value)
    return "store"


def partial_sink(view, rows, value):
    """A partial writer (an embedding backward: the rows of the ids only) always adds."""
    assert ops.grad_mode(view, False) is True
    view[rows] += value
    return "add"


def test_first_full_writer_stores_second_adds(arena):
    a, launches = arena
    ops.grad_begin(a)
    w = a[8:24].view(4, 4)
    assert full_sink(w, 1.0) == "store"
    assert full_sink(w, 0.5) == "add"                # a tied / shared parameter's second writer
    assert torch.equal(w, torch.full((4, 4), 1.5))
    assert launches == []                            # nothing had to be cleared for it
    assert K.grad_mode is ops.grad_mode              # the kernels' launches ask the same entry point


def test_full_writer_of_a_dense_permuted_view_stores_and_a_strided_one_adds(arena):
    a, launches = arena
    ops.grad_begin(a)
    conv = a[0:24].view(2, 3, 4).permute(0, 2, 1)    # dense in memory (a convolution weight's arena layout): a full view
    assert full_sink(conv, 1.0) == "store"
    cols = a[32:48].view(4, 4)[:, :2]                # 2 of 4 columns: covers its range in part only
    assert full_sink(cols, 1.0) == "add"
    assert launches == [[(32, 46)]]
    assert torch.equal(a[32:48].view(4, 4)[:, :2], torch.ones(4, 2)) and torch.equal(a[32:46].view(-1)[2:4], torch.zeros(2))


def test_self_overlapping_view_is_not_a_full_writer(arena):
    a, launches = arena
    ops.grad_begin(a)
    v = torch.as_strided(a, (3, 3), (2, 2), 8)       # 9 elements over a reach of 9, but positions 10, 12 twice and the odd ones never
    assert full_sink(v, 0.0) == "add"
    assert launches == [[(8, 17)]]


def test_plain_store_marks_its_range(arena):
    a, launches = arena
    ops.grad_begin(a)
    assert ops.grad_mode(a[0:8], True, store=True) is False      # accumulate=False: the launch overwrites ...
    a[0:8] = 5.0
    assert ops.grad_mode(a[0:8], True, store=True) is False      # ... also a second time
    assert full_sink(a[0:8], 1.0) == "add"
    _, unused = ops.grad_end()
    assert unused == [(8, 64)] and torch.equal(a[0:8], torch.full((8,), 6.0))


def test_peek_answers_without_marking(arena):
    a, launches = arena
    ops.grad_begin(a)
    assert ops.grad_mode(a[0:8], True, peek=True) is False and ops.grad_mode(a[0:8], False, peek=True) is True
    assert full_sink(a[0:8], 1.0) == "store" and ops.grad_mode(a[0:8], True, peek=True) is True
    assert launches == []


def test_partial_writer_before_any_full_writer_goes_on_the_pre_zero_list(arena):
    a, launches = arena
    ops.grad_begin(a)
    table = a[16:40].view(6, 4)
    partial_sink(table, [1, 3], 2.0)                 # cleared on demand, right before the launch
    assert launches == [[(16, 40)]]
    assert full_sink(table, 1.0) == "add"            # a full writer after it adds onto what is there
    demand, unused = ops.grad_end()
    assert demand == [(16, 40)]
    want = torch.ones(6, 4)
    want[[1, 3]] += 2.0
    assert torch.equal(table, want)
    # the next step of the structure clears the list up front, in ONE launch, and nothing on demand
    a.fill_(3.0)
    launches.clear()
    ops.grad_begin(a, demand)
    assert launches == [[(16, 40)]]
    partial_sink(table, [0], 2.0)
    assert launches == [[(16, 40)]]
    demand2, _ = ops.grad_end()
    assert demand2 == []


def test_full_writer_before_the_partial_writer_needs_no_clearing(arena):
    a, launches = arena
    ops.grad_begin(a)
    table = a[0:24].view(6, 4)                       # tied embedding: the output projection's weight gradient comes first
    assert full_sink(table, 1.0) == "store"
    partial_sink(table, [2], 2.0)
    assert launches == []
    assert float(table[2, 0]) == 3.0 and float(table[0, 0]) == 1.0


def test_view_written_by_nobody_lands_on_the_unused_list(arena):
    a, launches = arena
    ops.grad_begin(a)
    assert full_sink(a[8:16], 1.0) == "store"
    assert full_sink(a[40:48], 1.0) == "store"
    demand, unused = ops.grad_end()
    assert demand == [] and unused == [(0, 8), (16, 40), (48, 64)]
    assert launches == [[(0, 8), (16, 40), (48, 64)]]            # one launch, before the gradient norm reads the arena
    want = torch.zeros(64)
    want[8:16] = 1.0
    want[40:48] = 1.0
    assert torch.equal(a, want)                      # the unused-parameter rule: a zero gradient


def test_chunks_and_packed_views_are_ranges_not_names(arena):
    a, launches = arena
    ops.grad_begin(a)
    packed = a[0:48].view(12, 4)                     # three weights packed row-wise, written in chunks of rows (filler chunks)
    assert full_sink(packed[0:4], 1.0) == "store"
    assert full_sink(packed[4:12], 1.0) == "store"
    assert full_sink(packed, 1.0) == "add"           # the whole pack afterwards: everything under it is written
    assert full_sink(a[40:56], 1.0) == "add"         # half written, half not: the rest is cleared, then it adds
    assert launches == [[(48, 56)]]
    assert torch.equal(a[0:40], torch.full((40,), 2.0)) and torch.equal(a[40:48], torch.full((8,), 3.0))
    assert torch.equal(a[48:56], torch.ones(8))


def test_step_scalars_ride_in_the_pre_zero_launch(arena):
    a, launches = arena
    stats, gsq = torch.ones(3, dtype=torch.float64), torch.ones(1)
    ops.grad_begin(a, [(8, 16)], also=(stats, gsq))
    assert launches == [[(8, 16)]] and float(stats.sum()) == 0.0 and float(gsq) == 0.0
    assert full_sink(a[8:16], 1.0) == "add" and full_sink(a[0:8], 1.0) == "store"


def test_set_is_cleared_per_step(arena):
    a, launches = arena
    for _ in range(2):
        ops.grad_begin(a)
        assert full_sink(a[0:8], 1.0) == "store"     # the first writer of EVERY step stores
        assert full_sink(a[0:8], 1.0) == "add"
        ops.grad_end()
        assert torch.equal(a[0:8], torch.full((8,), 2.0))


def test_second_micro_batch_never_stores(arena):
    a, launches = arena
    ops.grad_begin(a)
    sinks = [a[0:16], a[16:32].view(4, 4), a[32:64]]
    assert [full_sink(v, 1.0) for v in sinks] == ["store"] * 3   # micro-batch 1
    assert [full_sink(v, 1.0) for v in sinks] == ["add"] * 3     # micro-batch 2: the same step, nothing is cleared in between
    ops.grad_end()
    assert launches == [] and torch.equal(a, torch.full((64,), 2.0))


def test_outside_a_step_and_outside_the_arena_every_sink_adds(arena):
    a, launches = arena
    other = torch.zeros(8)
    assert ops.grad_mode(a[0:8], True) is True       # no step is running
    ops.grad_begin(a)
    assert ops.grad_mode(other, True) is True        # not a view of the arena (an activation gradient's epilogue add)
    assert ops.grad_mode(a[0:8].double(), True) is True
    ops.grad_abort()                                 # a backward pass that raised
    assert ops.grad_mode(a[0:8], True) is True
    assert launches == []


def test_fold_queue_decides_at_its_flush(arena, monkeypatch):
    """A queued fold job asks when its launch is issued, not when it is queued: a writer launched in between is the first one."""
    a, launches = arena
    calls = []

    class _Lib:
        def call(self, name, *args):
            calls.append(name)

    monkeypatch.setattr(K, "lib", lambda: _Lib())
    monkeypatch.setattr(K, "stream", lambda: None)
    monkeypatch.setattr(K, "dptr", lambda t: t.data_ptr())
    ops.grad_begin(a)
    q = K.FoldQueue()
    part = torch.zeros(2, 8)
    q.add(part, 0, a[0:8], 8, 8, 2)
    q.add(part, 0, a[8:16], 8, 8, 2)
    assert full_sink(a[0:8], 1.0) == "store"         # launched before the flush
    jobs = list(q.jobs)
    q.flush()
    assert calls == ["ofa_fold_batched"]
    assert [j.accumulate & 1 for j in jobs] == [1, 0]


def test_tail_switch_is_a_debug_library_mask(monkeypatch):
    """OFA_STEP_TAIL_OLD (bit 0: first-touch off, the arena-wide fill of before) is read by libofasys_amd_dbg.so alone, at every call."""
    import ctypes
    import os
    from ofasys_amd import lib as L
    monkeypatch.setenv("OFA_STEP_TAIL_OLD", "1")
    if not L.LIB_PATH.endswith("_dbg.so"):
        assert K.tail_old(K.TAIL_FIRST_TOUCH) is False           # the product library has one path
    dbg = os.path.join(os.path.dirname(L.LIB_PATH), "libofasys_amd_dbg.so")
    assert os.path.exists(dbg), "build() makes the debug library next to the product library"
    fn = ctypes.CDLL(dbg).ofa_step_tail_old
    assert fn(0) == 1 and fn(1) == 0
    monkeypatch.setenv("OFA_STEP_TAIL_OLD", "0")
    assert fn(0) == 0
    monkeypatch.delenv("OFA_STEP_TAIL_OLD")
    assert fn(0) == 0
