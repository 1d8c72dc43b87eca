"""MCD evaluation measurements on the GPU (csrc/dtw.hip through ofasys_amd/mcd.py).
  DTW        both forms of ofa_dtw at every strip width the shape admits, and the distance form followed by ofa_dtw_backtrace, against a
             plain-torch restatement of the usual device formulation: one gather / min / scatter round per anti-diagonal over the padded
             [B, M, N] batch, then a backtrace on the host that reads one back pointer per path cell with .item().  The baseline's last DP
             cells are checked against the kernel's before anything is timed.
  MFCC       the MFCC pass (torch.stft + ofa_mfcc_rows) over 64 waveforms, and the gap of ofa_mfcc_rows against float64 numpy next to that
             of the same formula in float32 numpy.
  whole call batch_mel_cepstral_distortion on 32 pairs, host clock around the call (it ends in its one synchronisation).
Shapes: a ragged batch of 32 pairs of 200 .. 800 MFCC frames, and one 800 x 800 pair.  Every arm is warmed up; arms of one shape are timed
alternately in the same process, device events around `inner` calls; median and spread are printed.  Writes what it prints to
profiles/mcd_bench.txt (--out).  Usage: python tools/mcd_bench.py"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def spread(v):
    return f"median {statistics.median(v):10.3f} (min {min(v):.3f}, max {max(v):.3f}) ms"


def torch_dtw(dist, shapes):
    """The anti-diagonal loop in plain torch on the device, then the host backtrace.  -> (cum, bp, paths)."""
    B, m, n = dist.shape
    cum, bp = torch.zeros_like(dist), torch.full_like(dist, -1, dtype=torch.int32)
    cum[:, 0, :], cum[:, :, 0] = dist[:, 0, :].cumsum(-1), dist[:, :, 0].cumsum(-1)
    bp[:, 0, :], bp[:, :, 0] = 0, 2
    for k in range(2, m + n - 1):
        i = torch.arange(max(1, k - n + 1), min(m - 1, k - 1) + 1, device=dist.device)
        j = k - i
        v, a = torch.stack([cum[:, i, j - 1], cum[:, i - 1, j - 1], cum[:, i - 1, j]], dim=-1).min(dim=-1)
        bp[:, i, j] = a.int()
        cum[:, i, j] = v + dist[:, i, j]
    paths = []
    for b, (M, N) in enumerate(shapes):
        i, j, path = M - 1, N - 1, []
        while True:
            path.append((i, j))
            if i == 0 and j == 0:
                break
            code = bp[b, i, j].item()
            i, j = i - (code >= 1), j - (code <= 1)
        paths.append(path[::-1])
    return cum, bp, paths


def measure_dtw(tag, shapes, runs, inner, base_runs):
    from ofasys_amd import kernels as K, mcd
    B, maxM, maxN = len(shapes), max(s[0] for s in shapes), max(s[1] for s in shapes)
    gen = torch.Generator().manual_seed(B)
    x1, x2 = torch.randn(B, maxM, 16, generator=gen).cuda(), torch.randn(B, maxN, 16, generator=gen).cuda()
    x1[..., 13:], x2[..., 13:] = 0, 0
    dist = (torch.cdist(x1.double(), x2.double()).pow(2) / 13).sqrt().float().contiguous()
    sh = torch.tensor(shapes, dtype=torch.int32, device="cuda")
    arms = {}
    for c in (4, 8):
        if K.dtw_strip(True, maxN, c):
            arms[f"features form (rms, D = 13), strip {c}: total + pathlen"] = lambda c=c: K.dtw(sh, x1=x1, x2=x2, D=13, metric="rms", strip=c)
    for c in (4, 8, 16):
        if K.dtw_strip(False, maxN, c):
            arms[f"distance form, strip {c:2d}: + cumdist + backptr"] = lambda c=c: K.dtw(sh, distance=dist, want_cumdist=True, want_backptr=True, strip=c)
    arms["distance form (strip chosen) + ofa_dtw_backtrace, paths on the device"] = lambda: mcd.batch_dynamic_time_warping(dist, sh, return_path=False, pathmap=True)
    base = lambda: torch_dtw(dist, shapes)                                # noqa: E731
    cum_t, _, paths_t = base()
    total, pathlen, _, _ = K.dtw(sh, distance=dist)
    tf, _, _, _ = K.dtw(sh, x1=x1, x2=x2, D=13, metric="rms")
    same = all(float(cum_t[b, M - 1, N - 1]) == float(total[b]) for b, (M, N) in enumerate(shapes))
    rel = max(abs(float(tf[b]) - float(total[b])) / float(total[b]) for b in range(B))
    say(f"({tag}) B = {B} pairs, M {min(s[0] for s in shapes)} .. {maxM}, N {min(s[1] for s in shapes)} .. {maxN} frames, {sum(M * N for M, N in shapes)} cells "
        f"(padded {B * maxM * maxN}); {runs} alternated runs of {inner} calls, device events, ms per call")
    say(f"    torch loop's last DP cells equal the kernel's bit for bit: {same}; path lengths equal: "
        f"{[len(p) for p in paths_t] == pathlen.tolist()}; features form against distance form, largest relative difference of total {rel:.2e}")
    for fn in arms.values():
        timed(fn, 3)
    res = {k: [] for k in arms}
    for _ in range(runs):
        for k, fn in arms.items():
            res[k].append(timed(fn, inner))
    for k, v in res.items():
        say(f"    {k:78s}: {spread(v)}")
    tb = []
    for _ in range(base_runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        base()
        torch.cuda.synchronize()
        tb.append((time.perf_counter() - t0) * 1e3)
    say(f"    {'plain-torch anti-diagonal loop + host backtrace (host clock, ' + str(base_runs) + ' runs)':78s}: {spread(tb)}")
    best = min(statistics.median(v) for k, v in res.items() if k.startswith("distance form, strip"))
    say(f"    torch loop / distance form (best strip) = {statistics.median(tb) / best:.0f}x")


def measure_front_end(runs):
    from ofasys_amd import batch_mel_cepstral_distortion, kernels as K, mcd
    sr = 22050
    fn = mcd.MFCC(sr).cuda()
    rng = np.random.default_rng(1)
    lens = rng.integers(200 * fn.hop, 800 * fn.hop, 64).tolist()
    waves = [torch.from_numpy((0.1 * rng.standard_normal(n)).astype(np.float32)) for n in lens]
    batch = torch.nn.utils.rnn.pad_sequence(waves, batch_first=True).cuda()
    power = fn.power(batch, lens)
    say(f"(c) MFCC pass, {sr} Hz (n_fft {fn.n_fft}, hop {fn.hop}): 64 waveforms of {min(lens) / sr:.1f} .. {max(lens) / sr:.1f} s, "
        f"{power.shape[0] * power.shape[1]} padded frames; {runs} runs of 10 calls, device events, ms per call")
    arms = {"MFCC.forward: reflect pads + torch.stft + |X|^2 + ofa_mfcc_rows + tail mask": lambda: fn(batch, lens),
            "ofa_mfcc_rows alone (filter bank, log, DCT; one launch)": lambda: K.mfcc_rows(power, fn.filt_start, fn.filt_off, fn.filt_w, fn.dct)}
    for k, f in arms.items():
        timed(f, 3)
        say(f"    {k:78s}: {spread([timed(f, 10) for _ in range(runs)])}")
    # the gap of ofa_mfcc_rows on this power spectrum's first utterance against float64 numpy, next to float32 numpy's own
    p = power[0, :fn.num_frames(lens[0])].cpu().numpy()
    got = K.mfcc_rows(torch.from_numpy(p).cuda(), fn.filt_start, fn.filt_off, fn.filt_w, fn.dct).cpu().numpy()[:, :13]
    ref = {}
    for dt in (np.float64, np.float32):
        bank, dct = mcd.htk_mel_filters(sr, fn.n_fft).astype(dt), mcd.dct_table().astype(dt)
        ref[dt] = np.log(p.astype(dt) @ bank.T + dt(1e-6)) @ dct.T
    scale = np.abs(ref[np.float64]).max()
    say(f"    ofa_mfcc_rows against float64 numpy, largest error over the largest value: kernel {np.abs(got - ref[np.float64]).max() / scale:.3e}, "
        f"float32 numpy {np.abs(ref[np.float32] - ref[np.float64]).max() / scale:.3e}")
    y1, y2 = waves[:32], waves[32:]
    batch_mel_cepstral_distortion(y1, y2, sr)
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rets = batch_mel_cepstral_distortion(y1, y2, sr)
        ts.append((time.perf_counter() - t0) * 1e3)
    say(f"(d) batch_mel_cepstral_distortion, 32 pairs of these waveforms (host tensors in, host floats out; host clock, {runs} runs): {spread(ts)}")
    say(f"    mean MCD per path cell of the 32 noise pairs {statistics.mean(r[0] for r in rets):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcd_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mcd_bench.py needs a GPU: there is no fallback")
    say("tools/mcd_bench.py -- MCD evaluation: csrc/dtw.hip against a plain-torch anti-diagonal loop with a host backtrace")
    say(f"source_id {bench.source_id()}")
    with torch.no_grad():
        ragged = torch.randint(200, 801, (32, 2), generator=torch.Generator().manual_seed(5)).tolist()
        measure_dtw("a", [tuple(s) for s in ragged], runs=7, inner=20, base_runs=2)
        measure_dtw("b", [(800, 800)], runs=7, inner=20, base_runs=3)
        measure_front_end(runs=7)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
