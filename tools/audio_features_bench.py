"""Log-mel feature extraction measurements on the GPU (csrc/audio_features.hip through module/audio_features.py LogMelExtractor) against
torch's device composite over the padded batch, in float32: `unfold` (after the reflect pad, for tts), DC removal and pre-emphasis (kaldi),
window, `torch.fft.rfft`, the dense mel `matmul`, clamp and `log`.  The composite treats every utterance as full length; the kernel
takes the lengths.
  (a) kaldi  16 kHz, 80 mels, B = 32, ragged 2 .. 10 s                     (b) kaldi  16 kHz, one utterance of 10 s
  (c) tts    22.05 kHz, 1024 / 1024 / 256, 80 mels, B = 32, ragged 2 .. 10 s (d) tts    one utterance of 10 s
Both arms of a shape are warmed up, then timed alternately with device events in the same process; the spread is printed with the median.
Writes what it prints to profiles/audio_features_bench.txt (--out).  Usage: python tools/audio_features_bench.py"""
import argparse
import os
import statistics
import sys

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
    return f"median {statistics.median(v):9.3f} (min {min(v):.3f}, max {max(v):.3f}) ms"


def composite(ext, bank_t):
    """The same features from torch's own device operations, every utterance taken as full length."""
    N, win, shift, window = ext.n_fft, ext.win, ext.shift, ext.window

    def kaldi(wav):
        f = wav.unfold(-1, win, shift)
        f = f - f.mean(-1, keepdim=True)
        f = (f - 0.97 * torch.cat([f[..., :1], f[..., :-1]], dim=-1)) * window[:win]
        return (torch.fft.rfft(f, n=N).abs() ** 2 @ bank_t).clamp(min=1.1920929e-07).log()

    def tts(wav):
        x = torch.nn.functional.pad((wav * 2.0 ** -15).unsqueeze(1), (N // 2, N // 2), mode="reflect")[:, 0]
        return (torch.fft.rfft(x.unfold(-1, N, shift) * window).abs() @ bank_t).clamp(min=1e-5).log()
    return kaldi if ext.kind == "kaldi" else tts


def measure(tag, ext, bank, lens, runs, inner):
    B, L = len(lens), max(lens)
    wav = (torch.randn(B, L, generator=torch.Generator().manual_seed(B)) * 3000.0 + 500.0).cuda()
    comp = composite(ext, torch.as_tensor(bank, dtype=torch.float32).t().contiguous().cuda())
    arms = {"ours": lambda: ext(wav, lens if B > 1 else None)[0], "torch": lambda: comp(wav)}
    ours, ref = arms["ours"](), arms["torch"]()
    t0 = ext.num_frames(lens[0])
    d = float((ours[0, :t0] - ref[0, :t0]).abs().max()) if lens[0] == L else float("nan")
    say(f"({tag}) {ext.kind} {ext.sample_rate} Hz, window {ext.win}, shift {ext.shift}, n_fft {ext.n_fft}, {ext.n_mels} mels; B = {B}, "
        f"{min(lens) / ext.sample_rate:.1f} .. {L / ext.sample_rate:.1f} s, {sum(ext.num_frames(n) for n in lens)} frames (the padded batch has "
        f"{B * ext.num_frames(L)}); {runs} alternated runs of {inner} calls, device events, ms per call; utterance 0 (full length): max "
        f"difference of the two arms in the log domain {d:.2e}")
    for fn in arms.values():
        timed(fn, 3)
    res = {k: [] for k in arms}
    for _ in range(runs):
        for k, fn in arms.items():
            res[k].append(timed(fn, inner))
    say(f"    csrc/audio_features.hip, 1 launch (+ the lengths' upload)  : {spread(res['ours'])}")
    say(f"    float32 device composite over the padded batch             : {spread(res['torch'])}")
    say(f"    new path / composite = {statistics.median(res['ours']) / statistics.median(res['torch']):.3f} (medians; both include the host's launch work)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_features_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/audio_features_bench.py needs a GPU: there is no fallback")
    from ofasys_amd import LogMelExtractor
    from ofasys_amd.module.audio_features import kaldi_mel_banks
    from ofasys_amd.module.vocoder import mel_filters
    say("tools/audio_features_bench.py -- log-mel extraction of csrc/audio_features.hip against torch's float32 device composite")
    say(f"source_id {bench.source_id()}")
    with torch.no_grad():
        for tags, ext, bank in (("ab", LogMelExtractor.kaldi(16000, 80).cuda(), kaldi_mel_banks(16000, 512, 80)),
                                ("cd", LogMelExtractor.tts(22050, 1024, 256, 1024, 80, 0, 8000).cuda(), mel_filters(22050, 1024, 80, 0, 8000))):
            sr = ext.sample_rate
            lens = torch.randint(2 * sr, 10 * sr + 1, (32,), generator=torch.Generator().manual_seed(5)).tolist()
            lens[0] = 10 * sr
            measure(tags[0], ext, bank, lens, runs=7, inner=20)
            measure(tags[1], ext, bank, [10 * sr], runs=7, inner=50)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
