"""GPU: the EMA kernels (ofa_ema_step, ofa_ema_segments_step), the EMA object and TrainStep(ema=...) -- the kernels against the
recording of the reference's own EMA class update by update (tests/golden/ema.npz, tests/ema_case.py; each update starts from the
recording's previous state, so every bound is a single step's), the step against a host recomputation from parameter snapshots.

Bounds (units in the last place of the state's type):
  fp32 state    <= 1 from the recording: torch's CPU kernel fuses `add_(alpha=)`, the kernel is the unfused formula;
  16-bit state  <= 1 everywhere and at most 1 element in 1000 not bit-equal: a fused fp32 sum changes the 16-bit rounding only within
                one fp32 ulp of a tie (2^-15 of the elements for bf16, 2^-12 for fp16);
  decay 0       a bit-exact copy of the parameters;
  shadow        round(state), bit for bit.
"""
import os

import numpy as np
import pytest
import torch

from oracle.cases import CASES
from tests import ema_case as EC
from tests.golden_util import case_inputs
from tests.model_util import build_model, make_slots

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
KIND = {v: k for k, v in TORCH_DT.items()}
IDS = [EC.case_name(*c) for c in EC.CASES]
PAD = 16                                     # sentinel elements behind every arena: the kernels must not write past n


def to_dev(words, kind):
    """Storage words (tests/ema_case.py) -> a device tensor of that type."""
    if kind == "fp32":
        return torch.from_numpy(words.view(np.int32).copy()).view(torch.float32).to(DEV)
    return torch.from_numpy(words.view(np.int16).copy()).view(TORCH_DT[kind]).to(DEV)


def to_words(t):
    t = t.detach().contiguous().reshape(-1).cpu()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


def sentinel(n, kind):
    """n elements of a fixed bit pattern (finite, between 1.5 and 2 in every type, and no value any test writes)."""
    if kind == "fp32":
        return torch.full((n,), 0x3FC0DEAD, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full((n,), 0x3FED, dtype=torch.int16, device=DEV).view(TORCH_DT[kind])


def padded(words, kind):
    """The words on the device with PAD sentinel elements behind them -> (the n-element window, the whole buffer)."""
    buf = torch.cat([to_dev(words, kind), sentinel(PAD, kind)])
    return buf[:len(words)], buf


def sched_tensors(t, skip=0.0):
    return (torch.tensor([float(t)], dtype=torch.float64, device=DEV),
            torch.tensor([0.0, 0.0, 0.0, skip, 0.0], dtype=torch.float32, device=DEV))


def check_state(got, want, kind, what, full=True):
    dist = np.abs(EC.ordinal(got, kind) - EC.ordinal(want, kind))
    off = int((dist != 0).sum())
    print(f"MEASURED {what}: max distance {int(dist.max())} ulp, {off} of {len(got)} not bit-equal")
    assert dist.max() <= 1, what
    if kind != "fp32" and full:
        assert off * 1000 <= len(got), what


def run_update(c, p, u, n, start, freq, shadow, max_blocks=0):
    """Update u of a recorded case on the first n elements of `w`, from the recording's previous state -> (state, shadow) words."""
    from ofasys_amd import kernels as K
    skind, mkind = c["skind"], c["mkind"]
    state, sbuf = padded(c["state"]["w"][u][:n], skind)
    param, _ = padded(p[u + 1][:n], mkind)
    sh, shbuf = (None, None)
    if shadow:
        shbuf = sentinel(n + PAD, mkind)
        sh = shbuf[:n]
    step, sched = sched_tensors(u + 1)
    K.ema_step(state, param, sh, step, sched, EC.DECAY, start, freq, max_blocks=max_blocks)
    torch.cuda.synchronize()
    assert np.array_equal(to_words(sbuf[n:]), to_words(sentinel(PAD, skind))), "wrote behind the state"
    if shadow:
        assert np.array_equal(to_words(shbuf[n:]), to_words(sentinel(PAD, mkind))), "wrote behind the shadow"
    return to_words(state), (to_words(sh) if shadow else None)


@pytest.mark.parametrize("dt,fp32,start,freq", EC.CASES, ids=IDS)
def test_kernel_follows_the_recording_update_by_update(dt, fp32, start, freq):
    g = EC.load()
    c, p = g[EC.case_name(dt, fp32, start, freq)], g["params"][dt]["w"]
    skind = c["skind"]
    for u in range(EC.UPDATES):
        got, sh = run_update(c, p, u, EC.N_W, start, freq, shadow=True)
        want = c["state"]["w"][u + 1]
        if not c["applied"][u]:                                   # t % freq != 0: nothing is written, the shadow included
            assert np.array_equal(got, c["state"]["w"][u]) and np.array_equal(sh, to_words(sentinel(EC.N_W, dt)))
            continue
        check_state(got, want, skind, f"{EC.case_name(dt, fp32, start, freq)} update {u + 1}")
        assert np.array_equal(sh, EC.f32_to_words(EC.words_to_f32(got, skind), dt)), "shadow == round(state)"
        if c["decay"][u] == 0:
            assert np.array_equal(got, EC.f32_to_words(EC.words_to_f32(p[u + 1], dt), skind)), "decay 0 copies the parameters"


@pytest.mark.parametrize("dt,fp32", [(dt, f) for dt in EC.DTYPES for f in (False, True)])
def test_kernel_sizes_tails_and_grid_stride(dt, fp32):
    """n = 1, 3 (tail only), 4 (one quad), 7, 2053 (quads + tail, several blocks) and 5123 on TWO blocks -- a second grid-stride trip
    whose second quad is out of range, plus a tail -- with and without the shadow, on a decay-0.9 and a decay-0 update: each within
    the bound of the recording and bit-equal to the same elements of the full-size, default-grid run."""
    g = EC.load()
    for (start, freq), u in (((0, 1), 5), ((3, 1), 1)):
        c, p = g[EC.case_name(dt, fp32, start, freq)], g["params"][dt]["w"]
        assert c["applied"][u] and c["decay"][u] == (EC.DECAY if start == 0 else 0.0)
        full, full_sh = run_update(c, p, u, EC.N_W, start, freq, shadow=True)
        for n, mb in ((1, 0), (3, 0), (4, 0), (7, 0), (2053, 0), (EC.N_W, 2)):
            for shadow in (False, True):
                got, sh = run_update(c, p, u, n, start, freq, shadow, max_blocks=mb)
                check_state(got, c["state"]["w"][u + 1][:n], c["skind"], f"{dt} fp32={fp32} n={n} max_blocks={mb}", full=n == EC.N_W)
                assert np.array_equal(got, full[:n]), (n, mb, shadow)
                if shadow:
                    assert np.array_equal(sh, full_sh[:n])


@pytest.mark.parametrize("dt,fp32", [(dt, f) for dt in EC.DTYPES for f in (False, True)])
def test_skipped_or_off_frequency_updates_write_nothing(dt, fp32):
    from ofasys_amd import kernels as K
    skind = EC.state_kind(dt, fp32)
    n = 2053
    p = to_dev(EC.load()["params"][dt]["w"][1][:n], dt)
    for t, skip, freq, applies in ((4, 1.0, 1, False), (4, 0.0, 3, False), (5, 1.0, 5, False), (6, 0.0, 3, True)):
        state, shadow = sentinel(n, skind), sentinel(n, dt)
        step, sched = sched_tensors(t, skip)
        K.ema_step(state, p, shadow, step, sched, EC.DECAY, 0, freq)
        torch.cuda.synchronize()
        untouched = np.array_equal(to_words(state), to_words(sentinel(n, skind))) and np.array_equal(to_words(shadow), to_words(sentinel(n, dt)))
        assert untouched != applies, (t, skip, freq)


# the recording's BatchNorm buffers plus windows of 1, 5 and 1029 elements of `w`: (key, lo, hi) per segment
SEGS = [("bn.running_mean", 0, EC.N_BN), ("bn.running_var", 0, EC.N_BN), ("w", 0, 1), ("w", 1, 6), ("w", 6, 1035)]


@pytest.mark.parametrize("max_blocks", [0, 1])
@pytest.mark.parametrize("dt,fp32,start,freq", EC.CASES, ids=IDS)
def test_segments_kernel_follows_the_recording(dt, fp32, start, freq, max_blocks):
    """One launch over a device table: the default grid gives the 1029-element segment 5 blocks (the others leave at once), one block
    per segment strides over it."""
    from ofasys_amd import kernels as K
    g = EC.load()
    c = g[EC.case_name(dt, fp32, start, freq)]
    skind = c["skind"]
    segs = SEGS
    offs, total = [], 0
    for _, lo, hi in segs:
        offs.append(total)
        total += hi - lo
    for u in range(EC.UPDATES):
        srcs = [to_dev(g["params"][dt][k][u + 1][lo:hi].copy(), dt) for k, lo, hi in segs]
        state, sbuf = padded(np.concatenate([c["state"][k][u][lo:hi] for k, lo, hi in segs]), skind)
        shbuf = sentinel(total + PAD, dt)
        table, max_len = K.ema_segment_table(srcs, offs, torch.device(DEV))
        assert max_len == 1029
        step, sched = sched_tensors(u + 1)
        K.ema_segments_step(state, table, len(segs), max_len, shbuf[:total], TORCH_DT[dt], step, sched, EC.DECAY, start, freq,
                            max_blocks=max_blocks)
        torch.cuda.synchronize()
        got, sh = to_words(state), to_words(shbuf[:total])
        assert np.array_equal(to_words(sbuf[total:]), to_words(sentinel(PAD, skind))) and np.array_equal(to_words(shbuf[total:]), to_words(sentinel(PAD, dt)))
        if not c["applied"][u]:
            assert np.array_equal(sh, to_words(sentinel(total, dt)))
        want = np.concatenate([c["state"][k][u + 1][lo:hi] for k, lo, hi in segs])
        dist = np.abs(EC.ordinal(got, skind) - EC.ordinal(want, skind))
        assert dist.max() <= 1 and (skind == "fp32" or (dist != 0).sum() * 1000 <= total), u          # (1163 elements in all)
        if c["applied"][u]:
            assert np.array_equal(sh, EC.f32_to_words(EC.words_to_f32(got, skind), dt))


@pytest.mark.parametrize("dt,fp32", [(dt, f) for dt in EC.DTYPES for f in (False, True)])
def test_kernel_is_the_stated_formula_bit_for_bit_on_cancelling_values(dt, fp32):
    """The recording keeps every element's sign (tests/ema_case.py), so it never shows a state and a parameter of opposite sign.  Here
    they are independent draws -- half the sums cancel, some to a fraction of either term -- and the kernel must give the words of
    the unfused formula (`restate`, numpy) exactly: that formula is what the C ABI documents, and it leaves no rounding to choose."""
    from ofasys_amd import kernels as K
    skind = EC.state_kind(dt, fp32)
    rng = np.random.default_rng(7)
    n = 5123
    e = EC.f32_to_words(rng.standard_normal(n).astype(np.float32), skind)
    p = EC.f32_to_words((-EC.words_to_f32(e, skind) * 9 + rng.standard_normal(n).astype(np.float32) * 0.5).astype(np.float32), dt)
    p[::2] = EC.f32_to_words(rng.standard_normal((n + 1) // 2).astype(np.float32), dt)
    for decay, t, start in ((EC.DECAY, 3, 0), (0.9999, 3, 0), (EC.DECAY, 1, 2)):
        state, shadow = to_dev(e, skind), sentinel(n, dt)
        step, sched = sched_tensors(t)
        K.ema_step(state, to_dev(p, dt), shadow, step, sched, decay, start, 1)
        torch.cuda.synchronize()
        want = EC.restate(e, p, 0.0 if t < start else decay, skind, dt)
        assert np.array_equal(to_words(state), want), (decay, t, start)
        assert np.array_equal(to_words(shadow), EC.f32_to_words(EC.words_to_f32(want, skind), dt))


def test_segments_kernel_skips_a_record_that_leaves_the_state():
    from ofasys_amd import kernels as K
    src = [torch.ones(8, device=DEV), torch.ones(8, device=DEV)]
    state = torch.zeros(12, device=DEV)
    table, max_len = K.ema_segment_table(src, [0, 8], torch.device(DEV))           # the second would end at 16 > 12
    step, sched = sched_tensors(1)
    K.ema_segments_step(state, table, 2, max_len, None, torch.float32, step, sched, 0.0)
    torch.cuda.synchronize()
    assert state.tolist() == [1.0] * 8 + [0.0] * 4


class _Net(torch.nn.Module):
    """The module of the recording (tools/gen_ema_golden.py)."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(EC.N_W))
        self.bn = torch.nn.BatchNorm1d(EC.N_BN)
        self.register_buffer(EC.VERSION_KEY, torch.zeros(1))


def _set_net(net, g, dt, u):
    with torch.no_grad():
        sd = net.state_dict()
        for k in EC.FLOAT_KEYS:
            sd[k].copy_(to_dev(g["params"][dt][k][u], dt))
        sd[EC.INT_KEY].fill_(int(g["int"][dt][u]))
        sd[EC.VERSION_KEY].copy_(to_dev(g["version"][dt][u], dt))


@pytest.mark.parametrize("dt,fp32,start,freq", EC.CASES, ids=IDS)
def test_ema_object_follows_the_recording_through_every_kind_of_entry(dt, fp32, start, freq):
    """ema.EMA over the recording's module laid out by FlatParams: arena parameters (w, bn.weight, bn.bias), float buffers (one
    segments launch), the integer buffer (copied when, and only when, the average applies) and the "version" key (left alone).  The
    state is reloaded from the recording before every update, so the bound stays a single step's; the 16-bit cap counts over all
    5379 float elements of the module."""
    from ofasys_amd.ema import EMA, EMAConfig
    from ofasys_amd.trainer import FlatParams
    g = EC.load()
    c = g[EC.case_name(dt, fp32, start, freq)]
    skind = c["skind"]
    net = _Net().to(DEV).to(TORCH_DT[dt])
    _set_net(net, g, dt, 0)
    fp = FlatParams(net)
    step, sched = sched_tensors(0)
    ema = EMA(net, fp, EMAConfig(store_ema=True, ema_decay=EC.DECAY, ema_start_update=start, ema_update_freq=freq, ema_fp32=fp32), step_t=step)
    assert len(ema._groups) == 1 and sorted(ema._groups[0].keys) == sorted(EC.BUFFER_KEYS)
    sd = ema.state_dict()
    assert list(sd["ema"]) == list(net.state_dict()) and (sd["ema_fp32_params"] is not None) == fp32
    states = sd["ema_fp32_params"] if fp32 else sd["ema"]
    for k in EC.FLOAT_KEYS:                                                   # built as a copy of the model
        assert np.array_equal(to_words(states[k]), c["state"][k][0]), k
    for u in range(EC.UPDATES):
        with torch.no_grad():
            for k in EC.FLOAT_KEYS:                                           # every update from the recording's previous state
                states[k].copy_(to_dev(c["state"][k][u], skind))
        _set_net(net, g, dt, u + 1)
        step.fill_(u + 1)
        ema._enqueue(step, sched)
        torch.cuda.synchronize()
        off, total = 0, 0
        for k in EC.FLOAT_KEYS:
            got = to_words(states[k])
            dist = np.abs(EC.ordinal(got, skind) - EC.ordinal(c["state"][k][u + 1], skind))
            assert dist.max() <= 1, (k, u)
            off, total = off + int((dist != 0).sum()), total + len(got)
            if c["applied"][u]:
                assert np.array_equal(to_words(sd["ema"][k]), EC.f32_to_words(EC.words_to_f32(got, skind), dt)), (k, u)
        assert skind == "fp32" or off * 1000 <= total, (u, off)
        assert int(sd["ema"][EC.INT_KEY]) == int(c["int"][u + 1]), u
        assert np.array_equal(to_words(sd["ema"][EC.VERSION_KEY]), c["version"][u + 1]), u
        assert ema.get_decay() == float(c["decay"][u])
    sched[3] = 1.0                                                            # a skipped update: nothing moves, the integer included
    before = {k: to_words(v).copy() for k, v in states.items() if k in EC.FLOAT_KEYS}
    _set_net(net, g, dt, 0)
    ema._enqueue(step, sched)
    torch.cuda.synchronize()
    assert all(np.array_equal(before[k], to_words(states[k])) for k in before) and int(sd["ema"][EC.INT_KEY]) == int(c["int"][EC.UPDATES])


# ------------------------------------------------------------------------------------------------ inside the train step
EMA_CFG = dict(store_ema=True, ema_decay=0.9, ema_start_update=2, ema_fp32=True)


def _text_batches(d):
    """Two batch factories (fresh tensors per call: a captured step copies every later batch INTO the tensors it was captured with)."""
    vals, target = case_inputs(CASES["tiny_text"])

    def good():
        return {"slots": make_slots(vals, DEV, torch.bfloat16), "target": target.to(DEV)}

    def empty():                                           # only pad targets: sample_size = 0, the device guard skips the update
        return {"slots": make_slots(vals, DEV, torch.bfloat16), "target": torch.full_like(target, d.pad()).to(DEV)}
    return good, empty


def _host_step(prev, p, t, skipped, cfg):
    """The stated formula on the host, in numpy, from the previous fp32 state words and the model-dtype parameter words."""
    from ofasys_amd.ema import ema_schedule
    apply, decay = ema_schedule(t, skipped, cfg)
    return EC.restate(prev, p, decay, "fp32", "bf16") if apply else prev


def _run_steps(use_graph, freq, n_steps=6, skip_at=3, **kw):
    from ofasys_amd import ops
    from ofasys_amd.ema import as_config
    from ofasys_amd.trainer import TrainStep
    model, d = build_model(CASES["tiny_text"], DEV, torch.bfloat16)
    cfg = dict(EMA_CFG, ema_update_freq=freq)
    tr = TrainStep(model, lr=1e-3, clip_norm=1.0, use_graph=use_graph, graph_warmup=2, ema=cfg, **kw)
    good, empty = _text_batches(d)
    ops.manual_seed(5)
    t, worst, applied = 0, 0, 0
    for i in range(n_steps + (0 <= skip_at <= n_steps)):
        prev = to_words(tr.ema.state).copy()
        prev_shadow = to_words(tr.ema.shadow).copy()
        out = tr.train_step([empty() if i == skip_at else good()])
        torch.cuda.synchronize()
        skipped = bool(float(out["skipped"][0]))
        assert skipped == (i == skip_at)
        t += not skipped
        assert int(tr._step_t.item()) == t                      # a skipped update leaves the schedule where it was
        want = _host_step(prev, to_words(tr.fp.flat), t, skipped, as_config(cfg))
        got = to_words(tr.ema.state)
        if skipped or t % freq:
            assert np.array_equal(got, prev) and np.array_equal(to_words(tr.ema.shadow), prev_shadow), i
        else:
            applied += 1
            worst = max(worst, int(np.abs(EC.ordinal(got, "fp32") - EC.ordinal(want, "fp32")).max()))
            assert np.array_equal(to_words(tr.ema.shadow), EC.f32_to_words(EC.words_to_f32(got, "fp32"), "bf16"))
            if t < 2:
                assert np.array_equal(to_words(tr.ema.shadow), to_words(tr.fp.flat))      # before ema_start_update: a copy
    print(f"MEASURED train step graph={use_graph} freq={freq}: EMA state within {worst} fp32 ulp of the host recomputation over {applied} applied updates")
    assert worst <= 1 and applied == (n_steps // freq)
    return tr, model, d, good()


@pytest.mark.parametrize("freq", [1, 3])
@pytest.mark.parametrize("use_graph", [False, True])
def test_train_step_keeps_the_ema(use_graph, freq):
    """bf16 tiny text model, ema_fp32, decay 0.9, start 2: after every update the fp32 state equals the host recomputation from the
    previous state and a snapshot of the parameters the forward reads (within 1 fp32 ulp per step; independent of the training
    numerics).  The fourth batch has only pad targets: the device guard skips it, the EMA stays bit-unchanged and the schedule goes
    on from the same count.  With use_graph the last updates (the skipped one included) are replays of one captured graph."""
    tr, _, _, _ = _run_steps(use_graph, freq)
    if use_graph:
        assert tr.captured_graphs() == 1
        (entry,) = [e for e in tr._graphs.values() if "graphs" in e]
        assert tr.audit_report(entry) == [] or all("ema" not in name for name, *_ in tr.audit_report(entry))


def test_ema_off_launches_nothing_new():
    from ofasys_amd import kernels as K
    from ofasys_amd.trainer import TrainStep
    model, d = build_model(CASES["tiny_text"], DEV, torch.bfloat16)
    tr = TrainStep(model, lr=1e-3, ema={"store_ema": False, "ema_decay": 0.5})
    assert tr.ema is None
    good = _text_batches(d)[0]()
    calls = []
    orig = K.lib().call
    K.lib().call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        tr.train_step([good])
    finally:
        del K.lib().call
    torch.cuda.synchronize()
    assert "ofa_adam_step" in calls and not [c for c in calls if "ema" in c]


def test_shadow_model_reverse_and_restore():
    from ofasys_amd.trainer import FlatParams
    tr, model, d, good = _run_steps(False, 1, n_steps=4, skip_at=99)
    ema = tr.ema
    shadow_model = ema.get_model()
    assert shadow_model is ema.get_model() and not shadow_model.training
    assert all(not p.requires_grad for p in shadow_model.parameters())
    lo, hi = ema.shadow.data_ptr(), ema.shadow.data_ptr() + ema.shadow.numel() * ema.shadow.element_size()
    assert all(lo <= p.data_ptr() < hi for p in shadow_model.parameters() if p.numel())
    n_pack = 0
    for m_live, m in zip(model.modules(), shadow_model.modules()):
        packs = [getattr(m, "_pack", None) or {}] + ([m._cross_all[0]] if getattr(m, "_cross_all", None) is not None else [])
        live = [getattr(m_live, "_pack", None) or {}] + ([m_live._cross_all[0]] if getattr(m_live, "_cross_all", None) is not None else [])
        for pk, pl in zip(packs, live):
            for name in ("w", "b"):
                if torch.is_tensor(pl.get(name)):
                    n_pack += 1
                    assert lo <= pk[name].data_ptr() < hi and pk[name].shape == pl[name].shape
                    assert pk[name].data_ptr() - lo == pl[name].data_ptr() - tr.fp.flat.data_ptr()
            assert pk.get("gw") is None and pk.get("gb") is None
    assert n_pack >= 4                                        # the packed k|v|q windows and the all-layer cross k|v window exist
    model.eval()
    with torch.no_grad():
        live_logits = model(good["slots"])[0].float()
        ema_logits = shadow_model(good["slots"])[0].float()
        fresh, _ = build_model(CASES["tiny_text"], DEV, torch.bfloat16)
        fresh.load_state_dict({k: v.clone() for k, v in ema.state_dict()["ema"].items()})
        FlatParams(fresh)                                     # the same arena layout, hence the same packed GEMMs
        fresh.eval()
        fresh_logits = fresh(good["slots"])[0].float()
    assert torch.equal(ema_logits, fresh_logits) and not torch.equal(ema_logits, live_logits)
    # restore -> state_dict round-trips bit for bit, into the fp32 state too
    sd = {k: v.clone() for k, v in ema.state_dict()["ema"].items()}
    mod = {k: (v * 0.5 if v.is_floating_point() and "version" not in k else v.clone()) for k, v in sd.items()}
    ema.restore(mod, build_fp32_params=True)
    back = ema.state_dict()
    for k, v in mod.items():
        assert np.array_equal(to_words(back["ema"][k]) if v.is_floating_point() else back["ema"][k].cpu().numpy(),
                              to_words(v) if v.is_floating_point() else v.cpu().numpy()), k
        if v.is_floating_point() and "version" not in k:
            assert torch.equal(back["ema_fp32_params"][k], v.float()), k
    ema.restore(sd, build_fp32_params=True)
    with torch.no_grad():
        assert torch.equal(shadow_model(good["slots"])[0].float(), ema_logits)
    # reverse: the live model takes the averaged weights
    assert ema.reverse(model) is model
    with torch.no_grad():
        assert torch.equal(model(good["slots"])[0].float(), ema_logits)


def test_running_statistics_are_averaged_by_one_launch_per_update():
    """The tiny ResNet case: the BatchNorm running statistics (fp32 next to a bf16 model, outside the arena) are one segments launch
    per update, their state follows the host recomputation from snapshots; num_batches_tracked is copied."""
    from ofasys_amd import kernels as K
    from ofasys_amd.trainer import TrainStep
    case = CASES["tiny_resnet"]
    model, d = build_model(case, DEV, torch.bfloat16)
    vals, target = case_inputs(case)
    batch = {"slots": make_slots(vals, DEV, torch.bfloat16), "target": target.to(DEV)}
    tr = TrainStep(model, lr=1e-3, ema=dict(store_ema=True, ema_decay=0.9, ema_fp32=True))
    ema = tr.ema
    stats = [k for k in model.state_dict() if k.endswith("running_mean") or k.endswith("running_var")]
    groups = {id(ema._seg_of[k][0]) for k in stats}
    assert stats and len(groups) == 1
    calls = []
    orig = K.ema_segments_step
    K.ema_segments_step = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    try:
        for i in range(3):
            sd = ema.state_dict()
            prev = {k: to_words(sd["ema_fp32_params"][k]).copy() for k in stats}
            tr.train_step([batch])
            torch.cuda.synchronize()
            live = model.state_dict()
            for k in stats:
                want = EC.restate(prev[k], to_words(live[k]), 0.9, "fp32", KIND[live[k].dtype])
                got = to_words(sd["ema_fp32_params"][k])
                assert np.abs(EC.ordinal(got, "fp32") - EC.ordinal(want, "fp32")).max() <= 1, (k, i)
                assert np.array_equal(to_words(sd["ema"][k]), EC.f32_to_words(EC.words_to_f32(got, "fp32"), KIND[live[k].dtype])), k
            for k in live:
                if k.endswith("num_batches_tracked"):
                    assert int(sd["ema"][k]) == int(live[k])
    finally:
        K.ema_segments_step = orig
    assert len(calls) == 3 * len(ema._groups)
    with torch.no_grad():
        ema.get_model()(batch["slots"])                           # the averaged backbone runs on its averaged statistics
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ two ranks, sharded optimizer
def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    try:
        from ofasys_amd import ops
        from ofasys_amd.ema import as_config
        from ofasys_amd.trainer import TrainStep
        dev = f"cuda:{rank}"
        model, d = build_model(CASES["tiny_text"], dev, torch.bfloat16)
        cfg = dict(EMA_CFG, ema_update_freq=1)
        tr = TrainStep(model, lr=1e-3, clip_norm=1.0, shard_optimizer=True, bucket_bytes=1 << 16, ema=cfg)
        vals, target = case_inputs(CASES["tiny_text"])
        batch = {"slots": make_slots(vals, dev, torch.bfloat16), "target": target.roll(rank, 0).to(dev)}
        ops.manual_seed(5 + rank)
        worst = 0
        for t in range(1, 5):
            prev = to_words(tr.ema.state).copy()
            tr.train_step([batch])
            torch.cuda.synchronize()
            want = _host_step(prev, to_words(tr.fp.flat), t, False, as_config(cfg))
            worst = max(worst, int(np.abs(EC.ordinal(to_words(tr.ema.state), "fp32") - EC.ordinal(want, "fp32")).max()))
        q.put((rank, worst, to_words(tr.ema.state).copy(), to_words(tr.fp.flat).copy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL over xGMI)")
def test_two_ranks_with_a_sharded_optimizer_hold_the_same_ema():
    """shard_optimizer: every rank updates its share of the arena and gathers the rest; the EMA runs after the gather, so every rank
    averages the full parameters -- identical states, equal to the recomputation from each rank's own snapshots."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + os.getpid() % 1000
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in range(2)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, w0, s0, f0), (_, w1, s1, f1) = res
    assert w0 <= 1 and w1 <= 1
    assert np.array_equal(f0, f1) and np.array_equal(s0, s1)
