"""Generate tests/golden/ema.npz by RUNNING THE REFERENCE's EMA class (engine/ema/ema.py) on the CPU (build container only).

TEST INFRASTRUCTURE.  Usage:  python tools/gen_ema_golden.py
The cases, the module and the storage format are described in tests/ema_case.py.  Only data is stored: the recorded parameter /
buffer values, the decay the reference reported per update, which updates changed the EMA, and the EMA's state after every update
(as int8 distances from the unfused restatement, see tests/ema_case.py) with the CRC-32 of the reference's own words.
It also asserts what the tests rely on:
  * a state that did not change is bit-unchanged, and a decay-0 update is a bit-exact copy of the parameters;
  * every state is within 1 unit in the last place of the unfused restatement, and for 16-bit states at most 1 element in 1000
    differs at all (a fused fp32 sum changes the 16-bit rounding only within one fp32 ulp of a tie);
  * the model-dtype copy the reference keeps next to an fp32 state is that state rounded to the model dtype;
  * an fp32 model's state is the same with ema_fp32 on and off;
  * the integer buffer is copied, the "version" key is left alone.
"""
import dataclasses
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_import import install  # noqa: E402
from tests import ema_case as EC  # noqa: E402

TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(EC.N_W))
        self.bn = torch.nn.BatchNorm1d(EC.N_BN)
        self.register_buffer(EC.VERSION_KEY, torch.zeros(1))


def words(t):
    """A tensor's storage words as numpy (fp32 -> uint32, 16-bit -> uint16)."""
    t = t.detach().contiguous().reshape(-1)
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).copy()
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def kind_of(t):
    return {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}[t.dtype]


def values(seed):
    """UPDATES + 1 sets of fp32 values for every key (row 0: what the EMA is built from)."""
    g = torch.Generator().manual_seed(seed)
    out = []

    def signs(n):                       # fixed per element for the whole recording (tests/ema_case.py: no cancelling sums)
        return torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    sw, sb, sm = signs(EC.N_W), signs(EC.N_BN), signs(EC.N_BN)
    for u in range(EC.UPDATES + 1):
        out.append({"w": sw * (0.05 + torch.randn(EC.N_W, generator=g).abs()), "bn.weight": 1 + 0.3 * torch.rand(EC.N_BN, generator=g),
                    "bn.bias": sb * (0.05 + torch.randn(EC.N_BN, generator=g).abs()),
                    "bn.running_mean": sm * (0.05 + torch.randn(EC.N_BN, generator=g).abs()),
                    "bn.running_var": 0.5 + torch.rand(EC.N_BN, generator=g), EC.INT_KEY: torch.tensor(10 * u + 3),
                    EC.VERSION_KEY: torch.tensor([float(u + 1)])})
    return out


def set_model(model, vals):
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in vals.items():
            sd[k].copy_(v)


def main():
    install()
    from ofasys.configure.configs import EMAConfig
    from ofasys.engine.ema.ema import EMA
    # (the reference's dataclasses all inherit a private `_name` field from BaseDataclass: not an EMA option)
    out = {"defaults": np.array(json.dumps({k: v for k, v in dataclasses.asdict(EMAConfig()).items() if not k.startswith("_")}))}
    vals = values(20240607)
    fp32_states = {}
    worst_frac = {}
    for dt in EC.DTYPES:
        model = Net().to(TORCH_DT[dt])
        rec = {k: [] for k in EC.FLOAT_KEYS + (EC.INT_KEY, EC.VERSION_KEY)}
        for v in vals:
            set_model(model, v)
            for k, t in model.state_dict().items():
                rec[k].append(t.item() if k == EC.INT_KEY else words(t))
        for k in rec:
            out[f"p.{dt}.{k}"] = np.array(rec[k], dtype=np.int64) if k == EC.INT_KEY else np.stack(rec[k])
        for fp32 in (False, True):
            for start, freq in EC.SCHEDULES:
                name = EC.case_name(dt, fp32, start, freq)
                skind = EC.state_kind(dt, fp32)
                set_model(model, vals[0])
                cfg = EMAConfig(store_ema=True, ema_decay=EC.DECAY, ema_start_update=start, ema_update_freq=freq, ema_fp32=fp32)
                ema = EMA(model, cfg)

                def snapshot():
                    sd = ema.get_model().state_dict()
                    src = ema.fp32_params if fp32 else sd
                    st = {k: words(src[k]) for k in EC.FLOAT_KEYS}
                    for k in EC.FLOAT_KEYS:
                        assert kind_of(src[k]) == skind
                        # the model-dtype copy next to an fp32 state: that state, rounded
                        assert np.array_equal(words(sd[k]), EC.f32_to_words(EC.words_to_f32(st[k], skind), dt)), (name, k)
                    return st, int(sd[EC.INT_KEY]), words(sd[EC.VERSION_KEY])
                st0, i0, v0 = snapshot()
                states, ints, vers, decays, applied = [st0], [i0], [v0], [], []
                for u in range(EC.UPDATES):
                    set_model(model, vals[u + 1])
                    ema.step(model, updates=u + 1)
                    decays.append(float(ema.get_decay()))
                    st, i, v = snapshot()
                    changed = any(not np.array_equal(st[k], states[-1][k]) for k in EC.FLOAT_KEYS)
                    assert changed == all(not np.array_equal(st[k], states[-1][k]) for k in EC.FLOAT_KEYS)
                    applied.append(changed)
                    if changed:
                        assert i == 10 * (u + 1) + 3, "the integer buffer is copied"
                    else:
                        assert i == ints[-1]
                    assert np.array_equal(v, v0), 'a key containing "version" is left alone'
                    states.append(st)
                    ints.append(i)
                    vers.append(v)
                want = EC.ema_schedule_reference(start, freq, [False] * EC.UPDATES)
                assert [a for a, _ in want] == applied and [d for _, d in want] == decays, (name, want, applied, decays)
                out[f"{name}.decay"] = np.array(decays, dtype=np.float64)
                out[f"{name}.applied"] = np.array(applied, dtype=np.uint8)
                out[f"{name}.{EC.INT_KEY}"] = np.array(ints, dtype=np.int64)
                out[f"{name}.{EC.VERSION_KEY}"] = np.stack(vers)
                off, tot = [0] * EC.UPDATES, [0] * EC.UPDATES
                for k in EC.FLOAT_KEYS:
                    p = out[f"p.{dt}.{k}"]
                    deltas = np.zeros((EC.UPDATES, p.shape[1]), dtype=np.int8)
                    for u in range(EC.UPDATES):
                        if not applied[u]:
                            continue
                        got = states[u + 1][k]
                        if decays[u] == 0.0:
                            assert np.array_equal(got, EC.f32_to_words(EC.words_to_f32(p[u + 1], dt), skind)), "decay 0 copies"
                        base = EC.restate(states[u][k], p[u + 1], decays[u], skind, dt)
                        dlt = EC.ordinal(got, skind) - EC.ordinal(base, skind)
                        assert np.abs(dlt).max() <= 1, (name, k, u, np.abs(dlt).max())
                        if skind != "fp32":
                            off[u] += int((dlt != 0).sum())
                            tot[u] += dlt.size
                        deltas[u] = dlt
                    full = np.stack([states[u][k] for u in range(EC.UPDATES + 1)])
                    out[f"{name}.delta.{k}"] = deltas
                    out[f"{name}.crc.{k}"] = np.array(zlib.crc32(full.tobytes()), dtype=np.int64)
                    if dt == "fp32":
                        prev = fp32_states.setdefault((start, freq, k), full)
                        assert np.array_equal(prev, full), "an fp32 model's state does not depend on ema_fp32"
                if skind != "fp32":                 # the cap of the GPU tests, over all float elements of the module, per update
                    assert all(o * 1000 <= t for o, t in zip(off, tot)), (name, off, tot)
                    worst_frac[name] = max(off)
    np.savez_compressed(EC.PATH, **out)
    EC._cache = None
    g = EC.load()                                   # rebuilds every state and checks it against the recorded CRCs
    assert g["defaults"]["ema_decay"] == 0.9999
    print(f"wrote {EC.PATH}: {os.path.getsize(EC.PATH)} bytes; 16-bit states: elements off the unfused formula in the worst update: {worst_frac}")
    assert os.path.getsize(EC.PATH) <= 1 << 20


if __name__ == "__main__":
    main()
