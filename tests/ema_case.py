"""The EMA golden (tests/golden/ema.npz, written by tools/gen_ema_golden.py from the REFERENCE's own EMA class, engine/ema/ema.py)
and the numpy arithmetic its tests share.

The recording: a small module -- `w` (5123 floats), a BatchNorm1d(64) (two float parameters, two float buffers, one integer buffer) and
a float buffer whose key contains "version" -- takes 8 recorded sets of random values; after each, the reference's EMA.step(model,
updates) runs.  Every element keeps its sign through the recording (the signs are mixed across elements): the one-ulp bound between a
fused and an unfused `r + a * p` holds where the sum does not cancel, which an average of same-signed values never does.
The BatchNorm is 64 wide, a multiple of the CPU's vector length: torch's CPU kernel finishes a tensor's last partial vector in a scalar
loop whose 16-bit arithmetic (c10::Half / BFloat16 operators) also rounds the product a * p to the tensor's type -- 2 of 5 elements of
a 5-wide layer sat one ulp off the formula.  That is a property of that loop, not of the EMA; `w` keeps its 3 tail elements, which
stay inside the cap.
Every combination of model dtype {fp32, bf16, fp16} x ema_fp32 {False, True} x (ema_start_update, ema_update_freq) in {(0, 1), (3, 1),
(0, 3)} with ema_decay = 0.9.

Storage.  18 cases x 8 updates x 5123 states do not fit a committed file as raw words, so the state after an update is stored as
its distance, in units in the last place of the state's type, from `restate` below -- the UNFUSED two-rounding formula applied in
numpy to the reference's previous state and the recorded parameters.  The distances are int8 and almost all zero (torch's CPU kernel
may fuse `add_(alpha=)`).  The code is lossless: `load()` rebuilds the reference's words exactly and proves it against the CRC-32 of
each recorded array, taken from the reference's tensors when the file was written.
"""
import os
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "ema.npz")

N_W = 5123
N_BN = 64
UPDATES = 8
DECAY = 0.9
DTYPES = ("fp32", "bf16", "fp16")
SCHEDULES = ((0, 1), (3, 1), (0, 3))          # (ema_start_update, ema_update_freq)
CASES = [(dt, fp32, start, freq) for dt in DTYPES for fp32 in (False, True) for start, freq in SCHEDULES]
FLOAT_KEYS = ("w", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")
BUFFER_KEYS = ("bn.running_mean", "bn.running_var")
INT_KEY = "bn.num_batches_tracked"
VERSION_KEY = "ckpt_version"


def case_name(dt, fp32, start, freq):
    return f"{dt}.{'f32state' if fp32 else 'tstate'}.s{start}f{freq}"


def state_kind(dt, fp32):
    return "fp32" if fp32 else dt


# ---------------------------------------------------------------- words <-> values; kinds: "fp32" (uint32 words), "bf16", "fp16" (uint16)
def words_to_f32(words, kind):
    if kind == "fp32":
        return words.view(np.float32)
    if kind == "bf16":
        return (words.astype(np.uint32) << 16).view(np.float32)
    return words.view(np.float16).astype(np.float32)


def f32_to_words(x, kind):
    """Round-to-nearest-even to `kind` (finite values)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if kind == "fp32":
        return x.view(np.uint32).copy()
    if kind == "bf16":
        u = x.view(np.uint32).astype(np.uint64)
        u = u + 0x7FFF + ((u >> 16) & 1)
        return (u >> 16).astype(np.uint16)
    return x.astype(np.float16).view(np.uint16).copy()


def ordinal(words, kind):
    """A monotone integer image of the values: neighbours in the type differ by 1."""
    bits = 32 if kind == "fp32" else 16
    w = words.astype(np.int64)
    sign = w >> (bits - 1)
    mag = w & ((1 << (bits - 1)) - 1)
    return np.where(sign == 1, -mag, mag)


def from_ordinal(o, kind):
    bits = 32 if kind == "fp32" else 16
    w = np.where(o < 0, (-o) | (1 << (bits - 1)), o)
    return w.astype(np.uint32 if kind == "fp32" else np.uint16)


def restate(e_words, p_words, d, skind, mkind):
    """One applied update, unfused: e' = round_S(float(round_S(float(e) * d)) + a * float(p)); every product and the sum rounded to
    fp32 on its own (numpy does not contract).  a = fp32(1 - d) from Python's double -- and, for a 16-bit state, rounded once more
    to the state's type: torch's CPU `add_(alpha=)` converts the scalar to the tensor's dtype (bf16(0.1) = 0.10009765625), and that
    is the arithmetic the recording holds; `mul_` takes its scalar in fp32 for every dtype."""
    e = words_to_f32(e_words, skind)
    p = words_to_f32(p_words, mkind)
    d32, a32 = np.float32(d), np.float32(1.0 - d)
    a32 = words_to_f32(f32_to_words(np.array([a32]), skind), skind)[0]
    r = words_to_f32(f32_to_words(e * d32, skind), skind)
    return f32_to_words(r + a32 * p, skind)


def ema_schedule_reference(start, freq, skipped_flags):
    """The reference trainer + EMA.step as a state machine (trainer.py:931-939, ema.py:176-194): per attempted update, (applied, decay
    or None).  A skipped update advances neither num_updates nor the EMA's counter."""
    t, counter, out = 0, 0, []
    for skip in skipped_flags:
        if skip:
            out.append((False, None))
            continue
        t += 1
        decay = 0.0 if t < start else DECAY
        if freq > 1:
            counter += 1
            if counter >= freq:
                counter = 0
                out.append((True, decay))
            else:
                out.append((False, decay))
        else:
            out.append((True, decay))
    return out


def _crc(words):
    return zlib.crc32(np.ascontiguousarray(words).tobytes())


_cache = None


def load():
    """{"defaults": {...}, "params": {dt: {key: words [UPDATES + 1, n]}} (row 0: the values the EMA was built from),
    "int": {dt: [UPDATES + 1]}, "version": {dt: words [UPDATES + 1, 1]},
    case name: {"decay": [UPDATES], "applied": [UPDATES] bool, "state": {key: words [UPDATES + 1, n]} (row u + 1: after update u;
    row 0: the initial state), "int": [UPDATES + 1], "version": words [UPDATES + 1, 1] (of the EMA's model), "skind", "mkind"}}.
    Read-only: shared by every test."""
    global _cache
    if _cache is not None:
        return _cache
    import json
    z = np.load(PATH)
    out = {"defaults": json.loads(str(z["defaults"])), "params": {}, "int": {}, "version": {}}
    for dt in DTYPES:
        out["params"][dt] = {k: z[f"p.{dt}.{k}"] for k in FLOAT_KEYS}
        out["int"][dt] = z[f"p.{dt}.{INT_KEY}"]
        out["version"][dt] = z[f"p.{dt}.{VERSION_KEY}"]
    for dt, fp32, start, freq in CASES:
        name = case_name(dt, fp32, start, freq)
        skind = state_kind(dt, fp32)
        c = {"decay": z[f"{name}.decay"], "applied": z[f"{name}.applied"].astype(bool), "int": z[f"{name}.{INT_KEY}"],
             "version": z[f"{name}.{VERSION_KEY}"], "skind": skind, "mkind": dt, "state": {}}
        for k in FLOAT_KEYS:
            p = out["params"][dt][k]
            rows = [f32_to_words(words_to_f32(p[0], dt), skind)]          # the EMA starts as a copy of the model (ema.py:80, 117-126)
            delta = z[f"{name}.delta.{k}"]
            for u in range(UPDATES):
                if not c["applied"][u]:
                    rows.append(rows[-1])
                    continue
                base = restate(rows[-1], p[u + 1], float(c["decay"][u]), skind, dt)
                rows.append(from_ordinal(ordinal(base, skind) + delta[u], skind))
            st = np.stack(rows)
            assert _crc(st) == int(z[f"{name}.crc.{k}"]), f"tests/golden/ema.npz: {name}.{k} does not rebuild to the recorded words"
            st.setflags(write=False)
            c["state"][k] = st
        out[name] = c
    _cache = out
    return out
