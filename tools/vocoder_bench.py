"""HiFi-GAN vocoder measurements on the GPU (csrc/vocoder.hip through module/vocoder.py HiFiGANVocoder):
  (a) parity of the tiny generator of tests/test_vocoder_gpu.py: the relative error of the new path and of torch's device composite
      (F.conv1d / F.conv_transpose1d / F.leaky_relu in the same 16-bit dtype) against the float64 restatement, fp16 and bf16;
  (b) the HiFi-GAN v1 configuration (upsample_initial_channel 512, rates 8,8,2,2, kernels 16,16,4,4, resblock kernels 3,7,11, dilations
      1,3,5), fp16, seeded weights, one utterance of T = 800 frames: the new path against torch's device composite;
  (c) the same at a ragged batch of 32 utterances (lengths 200 .. 800 frames, the longest 800): the new path with `lengths=` against
      torch's composite over the padded batch (which computes the padding too, and whose utterances see their neighbours' padding).
Times are device events around `inner` back-to-back forwards after a warm-up, the two arms alternated in one process, median / min / max
over the runs; Gflop counts the generator's multiply-adds x 2 over the frames that exist.  Writes what it prints to
profiles/vocoder_bench.txt (--out).  Usage: python tools/vocoder_bench.py"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tests import vocoder_case as C  # noqa: E402

LINES = []


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def say(s):
    print(s, flush=True)
    LINES.append(s)


def spread(v):
    return f"median {statistics.median(v):8.3f} (min {min(v):.3f}, max {max(v):.3f}) ms"


def gflop_per_frame(cfg):
    """2 x multiply-adds of one input frame through the generator."""
    c0, hop, macs = cfg["upsample_initial_channel"], 1, 80 * cfg["upsample_initial_channel"] * 7
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        ch = c0 // 2 ** (i + 1)
        hop *= u
        macs += hop * 2 * ch * ch * k // u
        macs += hop * sum(2 * len(ds) * ch * ch * rk for rk, ds in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]))
    return 2 * (macs + hop * ch * 7) / 1e9


def vocoder(state, cfg, dtype):
    from ofasys_amd import HiFiGANVocoder
    voc = HiFiGANVocoder(None, cfg, dtype=dtype)
    voc.model.load_state_dict(state)
    return voc.cuda()


def parity():
    say("(a) the tiny generator (upsample_initial_channel 64, rates 2,2, resblock kernels 3,7), B = 2 ragged (12 and 7 frames), N(0, 1 / fan_in) weights: "
        "relative error (2-norm over both waveforms) against the float64 restatement, each utterance alone")
    state, gen, lens = C.generator_state(C.TINY), torch.Generator().manual_seed(1), (12, 7)
    x = torch.randn(2, 12, 80, generator=gen)
    want = torch.cat([C.generator({k: v.double() for k, v in state.items()}, C.TINY, x[b, :l].t()[None].double())[0, 0] for b, l in enumerate(lens)])
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        voc, xd = vocoder(state, C.TINY, dtype), x.to(dtype).cuda()
        got = voc(xd, lengths=lens)
        ours = torch.cat([got[b, 0, :4 * l] for b, l in enumerate(lens)])
        theirs = torch.cat([C.generator(state, C.TINY, xd[b, :l].t()[None])[0, 0] for b, l in enumerate(lens)])
        say(f"    {name}: csrc/vocoder.hip {C.rel(ours, want):.3e}, torch's device composite {C.rel(theirs.float(), want):.3e}")


def speed(tag, state, lens, runs, inner):
    dtype, T, B = torch.float16, max(lens), len(lens)
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(B, T, 80, generator=gen).to(dtype).cuda()
    for b, l in enumerate(lens):
        x[b, l:] = 0
    voc = vocoder(state, C.V1, dtype)
    dstate = {k: v.to(dtype).cuda() for k, v in state.items()}
    xt = x.transpose(1, 2).contiguous()
    lens_dev = torch.tensor(lens, dtype=torch.int32, device="cuda")
    arms = {"ours": lambda: voc.model.forward_rows(x, lens_dev if B > 1 else None), "torch": lambda: C.generator(dstate, C.V1, xt)}
    with torch.no_grad():
        a, b = arms["ours"](), arms["torch"]()[:, 0]
        diff = C.rel(torch.cat([a[i, :256 * l] for i, l in enumerate(lens)]), torch.cat([b[i, :256 * l] for i, l in enumerate(lens)]).float())
        for fn in arms.values():
            timed(fn, 2)
        res = {k: [] for k in arms}
        for _ in range(runs):
            for k, fn in arms.items():
                res[k].append(timed(fn, inner))
    gf = gflop_per_frame(C.V1) * sum(lens)
    say(f"({tag}) HiFi-GAN v1, fp16, B = {B}, frames {min(lens)} .. {T} ({sum(lens)} in all, {gf:.1f} Gflop over them; the padded batch has {B * T}); "
        f"{runs} alternated runs of {inner} forwards, device events, ms per forward; relative difference of the two arms' waveforms {diff:.2e}")
    say(f"    csrc/vocoder.hip, {2 + 4 * (1 + 18)} launches         : {spread(res['ours'])}  = {gf / statistics.median(res['ours']):.1f} Tflop/s over the frames that exist")
    say(f"    torch's device composite (padded)     : {spread(res['torch'])}")
    say(f"    new path / torch = {statistics.median(res['ours']) / statistics.median(res['torch']):.3f} (medians; both include the host's launch work)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocoder_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/vocoder_bench.py needs a GPU: there is no fallback")
    say("tools/vocoder_bench.py -- the HiFi-GAN vocoder of csrc/vocoder.hip against torch's device composite in the same 16-bit dtype")
    say(f"source_id {bench.source_id()}")
    with torch.no_grad():
        parity()
    state = C.generator_state(C.V1)
    speed("b", state, [800], runs=7, inner=5)
    lens = torch.randint(200, 801, (32,), generator=torch.Generator().manual_seed(5)).tolist()
    lens[0] = 800
    speed("c", state, lens, runs=5, inner=2)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
