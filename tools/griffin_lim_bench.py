"""Griffin-Lim vocoder measurements on the GPU (csrc/griffin_lim.hip through module/vocoder.py GriffinLimVocoder) at the reference's
configuration (n_fft 1024, window 1024, hop 256, 80 mels):
  (a) one `project` launch and (b) the whole vocoder (specgram, inverse, 32 project launches), each at one utterance of T = 800 frames and
      at a ragged batch of 32 (200 .. 800 frames), next to the float32 device composite of the reference's formulas (the dense Fourier
      bases of tests/test_griffin_lim_gpu.py's Restatement, atan2 / cos / sin, its window-sum-square made once; over the padded batch,
      which also computes the padding and reflects at the padded end).  The two strided convolutions are written as what they are --
      unfold + matmul and matmul + fold against the same bases -- so that they run as GEMMs: a 1024-tap conv1d is no shape a convolution
      library is built for.
Times are device events around `inner` back-to-back calls after a warm-up, the two arms alternated in one process, median / min / max over
the runs.  Writes what it prints to profiles/griffin_lim_bench.txt (--out).  Usage: python tools/griffin_lim_bench.py"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tests.test_griffin_lim_gpu import Restatement  # noqa: E402

N_FFT, WIN, HOP, ITERS = 1024, 1024, 256, 32
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


class Composite(Restatement):
    """The restatement in float32 on the device over a padded batch; the window-sum-square is made once per frame count."""

    def __init__(self, T, device="cuda"):
        from ofasys_amd.module.vocoder import window_sum_square
        super().__init__(N_FFT, WIN, HOP, torch.float32)
        self.wss = window_sum_square(self.window, T, HOP).to(device)
        self.fwd_t, self.inv_m = self.fwd[:, 0].t().contiguous().to(device), self.inv[:, 0].contiguous().to(device)     # [N, 2K], [2K, N]

    def project(self, w, S):                                             # w [B, L], S [B, K, T]
        x = torch.nn.functional.pad(w.unsqueeze(1), (N_FFT // 2, N_FFT // 2), mode="reflect")[:, 0]
        x = (x.unfold(-1, N_FFT, HOP) @ self.fwd_t).transpose(1, 2)      # the strided conv1d: frames [B, T, N] times the basis
        return self.inverse(S, torch.atan2(x[:, N_FFT // 2 + 1:], x[:, : N_FFT // 2 + 1]))

    def inverse(self, S, phase):
        y = torch.cat([S * torch.cos(phase), S * torch.sin(phase)], dim=1).transpose(1, 2) @ self.inv_m       # [B, T, N]
        n = N_FFT + HOP * (y.shape[1] - 1)                               # the strided conv_transpose1d: frames overlap-added by fold
        x = torch.nn.functional.fold(y.transpose(1, 2), (1, n), (1, N_FFT), stride=(1, HOP))[:, 0, 0]
        nz = self.wss > 1.1754944e-38
        x[:, nz] /= self.wss[nz]
        x *= N_FFT / HOP
        return x[:, N_FFT // 2: -(N_FFT // 2)]


def measure(tag, lens, runs, inner):
    from ofasys_amd import GriffinLimVocoder, kernels as K
    B, T, gen = len(lens), max(lens), torch.Generator().manual_seed(len(lens))
    voc = GriffinLimVocoder(22050, WIN, HOP, N_FFT, 80, 0, 8000, "hann", spec_bwd_max_iter=ITERS).cuda()
    comp = Composite(T)
    x = (torch.randn(B, T, 80, generator=gen) - 3.0).cuda()
    angles = ((torch.rand(B, N_FFT // 2 + 1, T, generator=gen) * 2 - 1) * torch.pi).cuda()
    frames = lens if B > 1 else None
    S = K.griffin_lim_specgram(x, voc.pinv_t)
    St, pinv = S.transpose(1, 2).contiguous(), voc.pinv_t.t().contiguous()
    tables = voc.tables(T, frames, "cuda")
    w0, out = K.griffin_lim_inverse(angles.transpose(1, 2).contiguous(), S, *tables), torch.empty(B, HOP * (T - 1), device="cuda")
    torch.cuda.synchronize()
    print(f"({tag}) inputs ready", flush=True)

    def composite_all():
        Sc = (pinv @ x.exp().transpose(1, 2)).clamp(min=0)
        w = comp.inverse(Sc, angles)
        for _ in range(ITERS):
            w = comp.project(w, Sc)
        return w
    arms = {"project": {"ours": lambda: K.griffin_lim_project(w0, S, *tables, out=out), "torch": lambda: comp.project(w0, St)},
            "vocoder": {"ours": lambda: voc(x, lengths=frames, angles=angles), "torch": composite_all}}
    d = (arms["project"]["ours"]()[0, :HOP * (lens[0] - 1)] - arms["project"]["torch"]()[0, :HOP * (lens[0] - 1)]).abs().max() / w0[0].abs().max()
    say(f"({tag}) B = {B}, frames {min(lens)} .. {T} ({sum(lens)} in all; the padded batch has {B * T}); {runs} alternated runs of {inner} calls, "
        f"device events, ms per call; one project step of utterance 0 (full length): max difference of the two arms {float(d):.2e} of max |w|")
    for what, pair in arms.items():
        for k, fn in pair.items():
            timed(fn, 1)
            print(f"    warmed up: {what} {k}", flush=True)
        res = {k: [] for k in pair}
        n = inner if what == "project" else max(1, inner // 8)
        for _ in range(runs):
            for k, fn in pair.items():
                res[k].append(timed(fn, n))
        launches = 1 if what == "project" else 2 + ITERS
        say(f"    {what:8s} csrc/griffin_lim.hip, {launches:2d} launch(es)   : {spread(res['ours'])}")
        say(f"    {what:8s} float32 device composite (padded) : {spread(res['torch'])}")
        say(f"    {what:8s} new path / composite = {statistics.median(res['ours']) / statistics.median(res['torch']):.3f} (medians; both include the host's launch work)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "griffin_lim_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/griffin_lim_bench.py needs a GPU: there is no fallback")
    say("tools/griffin_lim_bench.py -- the Griffin-Lim vocoder of csrc/griffin_lim.hip against the float32 device composite of the reference's formulas")
    say(f"source_id {bench.source_id()}; n_fft {N_FFT}, window {WIN}, hop {HOP}, 80 mels, {ITERS} iterations")
    with torch.no_grad():
        measure("a", [800], runs=7, inner=16)
        lens = torch.randint(200, 801, (32,), generator=torch.Generator().manual_seed(5)).tolist()
        lens[0] = 800
        measure("b", lens, runs=5, inner=8)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
