"""CPU: the EMA's host side -- configuration, Trainer plumbing, the schedule rule and the C ABI's refusals -- against the recording of
the reference's own EMA class (tests/golden/ema.npz, tests/ema_case.py)."""
import dataclasses
import inspect

import numpy as np
import pytest

from tests import ema_case as EC


def test_config_defaults_equal_the_references():
    from ofasys_amd.ema import EMAConfig
    assert dataclasses.asdict(EMAConfig()) == EC.load()["defaults"]
    assert [f.name for f in dataclasses.fields(EMAConfig)] == list(EC.load()["defaults"])


def test_trainer_plumbing():
    from ofasys_amd import Trainer, TrainerConfig
    from ofasys_amd.ema import EMAConfig, as_config
    from ofasys_amd.trainer import TrainStep
    t = Trainer()
    assert t.cfg.ema == EMAConfig() and t.ema is None and as_config(t.cfg.ema) is None          # off by default
    t = Trainer(store_ema=True, ema_decay=0.99, ema_fp32=True, ema_start_update=5, ema_update_freq=2, max_update=7)
    assert t.cfg.ema == EMAConfig(store_ema=True, ema_decay=0.99, ema_start_update=5, ema_update_freq=2, ema_fp32=True)
    assert t.cfg.optimization.max_update == 7 and t.ema is None                                 # (no step engine before setup)
    cfg = TrainerConfig()
    cfg.ema.store_ema = True
    assert Trainer(cfg).cfg.ema.store_ema
    with pytest.raises(TypeError, match="unknown trainer option"):
        Trainer(ema_momentum=0.5)
    assert inspect.signature(TrainStep.__init__).parameters["ema"].default is None
    # a dict works like the dataclass; store_ema off means no EMA whatever else is set
    assert as_config({"store_ema": True, "ema_decay": 0.5}) == EMAConfig(store_ema=True, ema_decay=0.5)
    assert as_config({"ema_decay": 0.5}) is None and as_config(None) is None
    with pytest.raises(ValueError, match="bad EMA configuration"):
        as_config(EMAConfig(store_ema=True, ema_update_freq=0))


def test_seed_model_is_refused():
    from ofasys_amd import Trainer
    from ofasys_amd.ema import EMAConfig, as_config
    with pytest.raises(NotImplementedError, match="ema_seed_model"):
        as_config(EMAConfig(store_ema=True, ema_seed_model="ema.pt"))
    with pytest.raises(NotImplementedError, match="ema_seed_model"):
        Trainer(store_ema=True, ema_seed_model="ema.pt")


@pytest.mark.parametrize("dt,fp32,start,freq", EC.CASES, ids=[EC.case_name(*c) for c in EC.CASES])
def test_schedule_reproduces_the_recording(dt, fp32, start, freq):
    """When the reference's state changed, and the decay it reported, update by update."""
    from ofasys_amd.ema import EMAConfig, ema_schedule
    c = EC.load()[EC.case_name(dt, fp32, start, freq)]
    cfg = EMAConfig(store_ema=True, ema_decay=EC.DECAY, ema_start_update=start, ema_update_freq=freq, ema_fp32=fp32)
    for u in range(EC.UPDATES):
        apply, decay = ema_schedule(u + 1, False, cfg)
        assert apply == bool(c["applied"][u]) and decay == float(c["decay"][u]), (u, apply, decay)
    assert c["applied"].any() and (start == 0 or (c["decay"][:start - 1] == 0).all())


@pytest.mark.parametrize("start,freq", EC.SCHEDULES)
def test_schedule_with_skipped_updates_interleaved(start, freq):
    """A skipped update advances neither the update count nor the reference's update_freq counter, and applies nothing."""
    from ofasys_amd.ema import EMAConfig, ema_schedule
    cfg = EMAConfig(store_ema=True, ema_decay=EC.DECAY, ema_start_update=start, ema_update_freq=freq)
    skipped = [False, True, False, False, True, True, False, False, False, True, False, False, False]
    want = EC.ema_schedule_reference(start, freq, skipped)
    t, applied = 0, 0
    for skip, (w_apply, w_decay) in zip(skipped, want):
        t += not skip                                  # the device's counter: step[0] after ofa_step_schedule
        apply, decay = ema_schedule(t, skip, cfg)
        assert apply == w_apply and (skip or decay == w_decay), (t, skip)
        applied += apply
    assert applied == (9 // freq)


def test_golden_is_within_the_stated_distance_of_the_unfused_formula():
    """What the GPU tests lean on: the recording sits within one unit in the last place of the two-rounding formula everywhere, and a
    16-bit state differs from it in at most 1 element in 1000 (load() has already proven the file rebuilds to the recorded words)."""
    g = EC.load()
    for case in EC.CASES:
        c = g[EC.case_name(*case)]
        p = g["params"][case[0]]["w"]
        st = c["state"]["w"]
        for u in range(EC.UPDATES):
            if not c["applied"][u]:
                assert np.array_equal(st[u + 1], st[u])
                continue
            base = EC.restate(st[u], p[u + 1], float(c["decay"][u]), c["skind"], c["mkind"])
            dist = np.abs(EC.ordinal(st[u + 1], c["skind"]) - EC.ordinal(base, c["skind"]))
            assert dist.max() <= 1
            if c["skind"] != "fp32":
                assert (dist != 0).mean() <= 1e-3
            if c["decay"][u] == 0:
                assert np.array_equal(st[u + 1], EC.f32_to_words(EC.words_to_f32(p[u + 1], case[0]), c["skind"]))


def test_abi_refusals_before_any_launch():
    from ofasys_amd import lib as L
    h = L.lib()
    P = 4096
    ok = dict(state=P, p=P, shadow=None, n=64, step=P, sched=P, decay=0.9, start=0, freq=1, dtype=L.BF16, sdtype=L.F32, mb=0)

    def call(**kw):
        a = dict(ok, **kw)
        h.call("ofa_ema_step", a["state"], a["p"], a["shadow"], a["n"], a["step"], a["sched"], a["decay"], a["start"], a["freq"],
               a["dtype"], a["sdtype"], a["mb"], None)
    with pytest.raises(L.OfaError, match="ema_step: bad dtype 7"):
        call(dtype=7)
    with pytest.raises(L.OfaError, match="the state is fp32 or of the model dtype"):
        call(dtype=L.BF16, sdtype=L.F16)
    with pytest.raises(L.OfaError, match="ema_step: bad argument"):
        call(sched=None)
    with pytest.raises(L.OfaError, match="update_freq >= 1"):
        call(freq=0)
    with pytest.raises(L.OfaError, match="decay in"):
        call(decay=1.5)
    with pytest.raises(L.OfaError, match="16-byte"):
        call(state=P + 8)                              # an fp32 state needs 16 bytes
    with pytest.raises(L.OfaError, match="16-byte"):
        call(p=P + 4)                                  # a 16-bit arena needs 8
    with pytest.raises(L.OfaError, match="16-byte"):
        call(shadow=P + 2)
    with pytest.raises(L.OfaError, match="at most 65535 segments"):
        h.call("ofa_ema_segments_step", P, P, None, 70000, 10, 5, P, P, 0.9, 0, 1, L.F32, L.F32, 0, None)
    with pytest.raises(L.OfaError, match="ema_segments_step: bad dtype"):
        h.call("ofa_ema_segments_step", P, P, None, 1, 10, 5, P, P, 0.9, 0, 1, 9, L.F32, 0, None)


@pytest.mark.parametrize("name", ["tiny_text", "tiny_resnet"])
def test_shadow_model_holds_no_reference_to_the_live_model(name):
    """get_model() (no kernel runs: the layout is host work): every parameter and every packed attention window of the copy lies in
    the shadow arena at the live arena's offset, buffers are the EMA's own, and no closure, list or attribute of the copy still
    reaches a module or tensor of the live model -- copy.deepcopy copies functions by reference, and the adaptors reach the shared
    token embedding through closures: a copy that kept them would embed and project with the LIVE weights."""
    import types

    import torch
    from oracle.cases import CASES
    from ofasys_amd.ema import EMA, EMAConfig
    from ofasys_amd.trainer import FlatParams
    from tests.model_util import build_model
    model, _ = build_model(CASES[name], None, torch.bfloat16)
    fp = FlatParams(model)
    ema = EMA(model, fp, EMAConfig(store_ema=True, ema_fp32=True))
    copy_ = ema.get_model()
    assert copy_ is ema.get_model() and not copy_.training and not any(p.requires_grad for p in copy_.parameters())
    lo, hi = ema.shadow.data_ptr(), ema.shadow.data_ptr() + ema.shadow.numel() * 2
    in_arena = {k for k, v in ema._kind.items() if v == "arena"}
    live_sd, sd = model.state_dict(), copy_.state_dict()
    assert list(sd) == list(live_sd)
    for k in sd:
        assert torch.equal(sd[k], live_sd[k]) and (sd[k].numel() == 0 or sd[k].data_ptr() != live_sd[k].data_ptr()), k
        if k in in_arena:
            assert sd[k].data_ptr() - lo == live_sd[k].data_ptr() - fp.flat.data_ptr() and sd[k].stride() == live_sd[k].stride(), k
    live_mods = {id(m) for m in model.modules()}
    live_tensors = {id(t) for t in list(model.parameters()) + list(model.buffers())}
    packs = 0
    for (mod_name, mod), live_mod in zip(copy_.named_modules(), model.modules()):
        for k, v in vars(mod).items():
            cells = [c.cell_contents for c in (v.__closure__ or ())] if isinstance(v, types.FunctionType) else []
            items = list(v) if isinstance(v, (list, tuple)) else []
            for x in cells + items + [v]:
                assert id(x) not in live_mods and id(x) not in live_tensors, (mod_name, k)
        for pack, live_pack in ((getattr(mod, "_pack", None), getattr(live_mod, "_pack", None)),
                                ((getattr(mod, "_cross_all", None) or (None,))[0], (getattr(live_mod, "_cross_all", None) or (None,))[0])):
            for key in ("w", "b"):
                if live_pack and torch.is_tensor(live_pack.get(key)):
                    packs += 1
                    assert lo <= pack[key].data_ptr() < hi and pack[key].data_ptr() - lo == live_pack[key].data_ptr() - fp.flat.data_ptr()
                    assert pack.get("gw") is None and pack.get("gb") is None
    assert packs >= 4
