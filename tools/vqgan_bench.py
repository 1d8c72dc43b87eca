"""VQGAN image decoder measurements on the GPU (csrc/vqgan.hip through module/vqgan.py VQGANTokenizer):
  (a) the errors of tests/test_vqgan_gpu.py's prologue chain and tiny decoder: the new path and torch's device composite (F.group_norm ->
      swish -> F.conv2d in the same 16-bit dtype) against the float64 restatement;
  (b) the f8 Gumbel configuration (ch 128, ch_mult 1,1,2,4, two res blocks, attention at 32 x 32, 256 x 256 output), seeded weights, bf16 and
      fp16 at B = 1 and B = 8: `decode_code` against torch's device composite of the same decoder from the same state dict;
  (c) one vq_conv3x3 launch at 256 x 256 x 128 -> 128 and at 32 x 32 x 512 -> 512 (B = 1, bf16) against F.conv2d, NCHW and channels_last.
Times are device events around `inner` back-to-back calls after a warm-up, the arms alternated in one process, median / min / max over the
runs; Gflop counts 2 x the multiply-adds of the convolutions and of the attention products.  Writes what it prints to
profiles/vqgan_bench.txt (--out).  Usage: python tools/vqgan_bench.py

`--arm encode` measures the encoder instead (csrc/vqgan_encode.hip through VQGANTokenizer(with_encoder=True)) and writes
profiles/vqgan_encode_bench.txt:
  (d) the f8 encoder, 256 x 256 images -> 32 x 32 codes, bf16 and fp16 at B = 1 and B = 8: `encode` with and without the Gumbel noise against
      torch's device composite of tests/vqgan_encode_case.py (the restated Encoder, quant_conv, the proj convolution and, as the reference,
      F.gumbel_softmax(hard) -> argmax);
  (e) the quantize launch alone at N = 8192, K = 256, n_embed = 8192 against F.conv2d + argmax."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tests import vqgan_case as C  # noqa: E402

LINES = []
DTYPES = (("bf16", torch.bfloat16), ("fp16", torch.float16))


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def spread(v):
    return f"median {statistics.median(v):8.3f} (min {min(v):.3f}, max {max(v):.3f}) ms"


def say(s):
    print(s, flush=True)
    LINES.append(s)


def gflop_per_image(cfg):
    """2 x multiply-adds of one image through post_quant_conv and the Decoder."""
    dd = cfg["ddconfig"]
    chans, levels = [dd["ch"] * m for m in dd["ch_mult"]], len(dd["ch_mult"])
    side = dd["resolution"] // 2 ** (levels - 1)
    res = lambda ci, co: 9 * ci * co + 9 * co * co + (ci * co if ci != co else 0)          # noqa: E731  (per pixel)
    attn = lambda c, px: 4 * c * c + 2 * px * c                                              # noqa: E731  (per pixel)
    c = chans[-1]
    macs = side * side * (cfg["embed_dim"] * dd["z_channels"] + 9 * dd["z_channels"] * c + 2 * res(c, c) + attn(c, side * side))
    for i in reversed(range(levels)):
        for _ in range(dd["num_res_blocks"] + 1):
            macs += side * side * (res(c, chans[i]) + (attn(chans[i], side * side) if side in dd["attn_resolutions"] else 0))
            c = chans[i]
        if i:
            side *= 2
            macs += side * side * 9 * c * c
    return 2 * (macs + side * side * 9 * c * dd["out_ch"]) / 1e9


def count_calls(fn):
    """C-ABI calls of one fn() (a statistics call is two kernels: partial sums and the finalise)."""
    from ofasys_amd.lib import lib
    calls, orig = [], lib().call
    lib().call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        fn()
    finally:
        del lib().call
    return len(calls), sum(n == "ofa_vqgan_groupnorm_stats" for n in calls)


def parity():
    from tests import test_vqgan_gpu as G
    say("(a) relative error (2-norm) against the float64 restatement on the same rounded inputs: csrc/vqgan.hip, then torch's device composite")
    for kind, name, Cin, Cout, up in G.PROLOGUE:
        x, gamma, beta, w, b = G._operands(torch.Generator().manual_seed(Cin + Cout), kind, G.DTYPES[name], Cin, Cout, 19, 35)
        want = C.conv3x3(x.double().cpu(), w.double().cpu(), b.double().cpu(), norm=(gamma.double().cpu(), beta.double().cpu()), up=up)
        say(f"    groupnorm_stats + conv3x3, {kind:6s} {name} {Cin:3d} -> {Cout:3d}{' x2' if up else '   '} 19 x 35, B = 2: "
            f"{C.rel(G._chain(x, gamma, beta, w, b, up=up), want):.3e}, {C.rel(C.conv3x3(x, w, b, norm=(gamma, beta), up=up), want):.3e}")
    from ofasys_amd import VQGANTokenizer
    for name, dtype in DTYPES:
        tok = VQGANTokenizer(C.TINY, None, code_image_size=16, vqgan_factor=2, dtype=dtype)
        codes = torch.randint(0, 64, (2, 8, 8), generator=torch.Generator().manual_seed(1))
        state = tok.vqgan.state_dict()
        want = C.decode_code({k: v.double().cpu() for k, v in state.items()}, C.TINY, codes, torch.zeros(1, dtype=torch.float64))
        say(f"    the tiny decoder (ch 32, ch_mult 1,2, one res block, attention at 8 x 8, 16 x 16 output), {name}, B = 2: "
            f"{C.rel(tok.vqgan.decode_code(codes), want):.3e}, {C.rel(C.decode_code(state, C.TINY, codes, state['post_quant_conv.bias']), want):.3e}")


def decoder_speed(name, dtype, B, runs, inner):
    from ofasys_amd import VQGANTokenizer
    tok = VQGANTokenizer(C.F8, None, dtype=dtype)
    state = tok.vqgan.state_dict()
    codes = torch.randint(0, C.F8["n_embed"], (B, 32, 32), generator=torch.Generator().manual_seed(B)).cuda()
    arms = {"ours": lambda: tok.vqgan.decode_code(codes), "torch": lambda: C.decode_code(state, C.F8, codes, state["post_quant_conv.bias"])}
    diff = C.rel(arms["ours"](), arms["torch"]().float())
    calls, stats = count_calls(arms["ours"])
    for fn in arms.values():
        timed(fn, 1)
    res = {k: [] for k in arms}
    for _ in range(runs):
        for k, fn in arms.items():
            res[k].append(timed(fn, inner))
    gf, ours, theirs = gflop_per_image(C.F8) * B, statistics.median(res["ours"]), statistics.median(res["torch"])
    say(f"    {name}, B = {B} ({gf:.1f} Gflop); {runs} alternated runs of {inner} decodes, ms per decode; relative difference of the two arms' images {diff:.2e}")
    say(f"        csrc/vqgan.hip, {calls} calls ({calls + stats} kernels): {spread(res['ours'])} = {ours / B:.3f} ms per image, {gf / ours:.1f} Tflop/s")
    say(f"        torch's device composite              : {spread(res['torch'])} = {theirs / B:.3f} ms per image")
    say(f"        new path / torch = {ours / theirs:.3f} (medians; both include the host's launch work)")


def conv_speed(H, Cn, runs, inner):
    from ofasys_amd import ops
    from ofasys_amd.module.vqgan import tap_major2d
    gen, dtype = torch.Generator().manual_seed(Cn), torch.bfloat16
    x = torch.randn(1, Cn, H, H, generator=gen).to(dtype).cuda()
    w, b = (torch.randn(Cn, Cn, 3, 3, generator=gen) / (9 * Cn) ** 0.5).to(dtype).cuda(), torch.zeros(Cn, dtype=dtype, device="cuda")
    xr, w9, xl, wl = C.rows(x), tap_major2d(w), x.contiguous(memory_format=torch.channels_last), w.contiguous(memory_format=torch.channels_last)
    arms = {"ours": lambda: ops.vqgan_conv3x3(xr, w9, b), "nchw": lambda: F.conv2d(x, w, b, padding=1), "nhwc": lambda: F.conv2d(xl, wl, b, padding=1)}
    diff = C.rel(arms["ours"]().permute(0, 3, 1, 2), arms["nchw"]())
    for fn in arms.values():
        timed(fn, 3)
    res = {k: [] for k in arms}
    for _ in range(runs):
        for k, fn in arms.items():
            res[k].append(timed(fn, inner))
    gf, ours = 2 * 9 * Cn * Cn * H * H / 1e9, statistics.median(res["ours"])
    say(f"    {H} x {H} x {Cn} -> {Cn}, bf16, B = 1 ({gf:.1f} Gflop); {runs} alternated runs of {inner} launches; relative difference {diff:.2e}")
    say(f"        vq_conv3x3 (no prologue)     : {spread(res['ours'])} = {gf / ours:.1f} Tflop/s")
    say(f"        F.conv2d, NCHW               : {spread(res['nchw'])}; vq_conv3x3 / F.conv2d = {ours / statistics.median(res['nchw']):.3f}")
    say(f"        F.conv2d, channels_last      : {spread(res['nhwc'])}; vq_conv3x3 / F.conv2d = {ours / statistics.median(res['nhwc']):.3f}")


def alternate(arms, runs, inner):
    for fn in arms.values():
        timed(fn, 1)
    res = {k: [] for k in arms}
    for _ in range(runs):
        for k, fn in arms.items():
            res[k].append(timed(fn, inner))
    return res


def encoder_speed(name, dtype, B, runs, inner):
    from ofasys_amd import VQGANTokenizer
    from tests import vqgan_encode_case as E
    tok = VQGANTokenizer(C.F8, None, dtype=dtype, with_encoder=True)
    state = tok.vqgan.state_dict()
    x = torch.randn(B, 3, 256, 256, generator=torch.Generator().manual_seed(B)).to(dtype).float().cuda()
    xt, pw, pb = x.to(dtype), state["quantize.proj.weight"], state["quantize.proj.bias"]
    arms = {"ours": lambda: tok.encode(x, seed=1), "plain": lambda: tok.encode(x, gumbel=False),
            "torch": lambda: F.gumbel_softmax(F.conv2d(E.prequant(state, C.F8, xt), pw, pb), tau=1.0, dim=1, hard=True).argmax(1)}
    diff = C.rel(tok.encode_to_prequant(x), E.prequant(state, C.F8, xt).float())
    same = float((arms["plain"]() == F.conv2d(E.prequant(state, C.F8, xt), pw, pb).argmax(1).view(B, -1)).float().mean())
    calls, stats = count_calls(arms["ours"])
    res = alternate(arms, runs, inner)
    ours, theirs = statistics.median(res["ours"]), statistics.median(res["torch"])
    say(f"    {name}, B = {B}; {runs} alternated runs of {inner} encodes, ms per encode; relative difference of the two arms' pre-quant features {diff:.2e}, "
        f"equal plain arg-max codes {100 * same:.1f} %")
    say(f"        csrc/vqgan_encode.hip + vqgan.hip, {calls} calls ({calls + stats} kernels + the split fold), Gumbel noise: {spread(res['ours'])} = {ours / B:.3f} ms per image")
    say(f"        the same without the noise                      : {spread(res['plain'])}")
    say(f"        torch's device composite (F.gumbel_softmax hard): {spread(res['torch'])} = {theirs / B:.3f} ms per image")
    say(f"        new path / torch = {ours / theirs:.3f} (medians; both include the host's launch work)")


def quantize_speed(runs, inner):
    from ofasys_amd import ops
    N, Kd, n_embed, gen, dtype = 8192, 256, 8192, torch.Generator().manual_seed(0), torch.bfloat16
    h, w = torch.randn(N, Kd, generator=gen).to(dtype).cuda(), (torch.randn(n_embed, Kd, generator=gen) / Kd ** 0.5).to(dtype).cuda()
    b = (0.1 * torch.randn(n_embed, generator=gen)).to(dtype).cuda()
    hn, w4 = h.view(8, 32, 32, Kd).permute(0, 3, 1, 2).contiguous(), w.view(n_embed, Kd, 1, 1)
    arms = {"ours": lambda: ops.vqgan_quantize(h, w, b), "noise": lambda: ops.vqgan_quantize(h, w, b, 1), "torch": lambda: F.conv2d(hn, w4, b).argmax(1)}
    same = float((arms["ours"]() == arms["torch"]().view(-1)).float().mean())
    res = alternate(arms, runs, inner)
    gf, ours = 2 * N * Kd * n_embed / 1e9, statistics.median(res["ours"])
    say(f"    N = {N}, K = {Kd}, n_embed = {n_embed}, bf16 ({gf:.1f} Gflop); {runs} alternated runs of {inner} calls; codes equal to torch's {100 * same:.2f} % "
        "(torch rounds the logits to bf16 before its arg-max)")
    say(f"        vq_quantize + fold, no noise : {spread(res['ours'])} = {gf / ours:.1f} Tflop/s")
    say(f"        vq_quantize + fold, noise    : {spread(res['noise'])}")
    say(f"        F.conv2d + argmax            : {spread(res['torch'])}; vq_quantize / torch = {ours / statistics.median(res['torch']):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("decode", "encode"), default="decode")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "vqgan_bench.txt" if args.arm == "decode" else "vqgan_encode_bench.txt")
    if not torch.cuda.is_available():
        raise SystemExit("tools/vqgan_bench.py needs a GPU: there is no fallback")
    if args.arm == "encode":
        say("tools/vqgan_bench.py --arm encode -- the VQGAN encoder of csrc/vqgan_encode.hip against torch's device composite in the same 16-bit dtype")
        say(f"source_id {bench.source_id()}")
        with torch.no_grad():
            say("(d) the f8 Gumbel encoder (ch 128, ch_mult 1,1,2,4, two res blocks, attention at 32 x 32), 256 x 256 images -> 32 x 32 codes, seeded weights, device events")
            for name, dtype in DTYPES:
                encoder_speed(name, dtype, 1, runs=7, inner=3)
                encoder_speed(name, dtype, 8, runs=5, inner=1)
            say("(e) the quantizer alone against F.conv2d + argmax, device events, ms per call")
            quantize_speed(runs=7, inner=10)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
        return
    say("tools/vqgan_bench.py -- the VQGAN decoder of csrc/vqgan.hip against torch's device composite in the same 16-bit dtype")
    say(f"source_id {bench.source_id()}")
    with torch.no_grad():
        parity()
        say("(b) the f8 Gumbel decoder (ch 128, ch_mult 1,1,2,4, two res blocks, attention at 32 x 32), 32 x 32 codes -> 256 x 256 images, seeded weights, device events")
        for name, dtype in DTYPES:
            decoder_speed(name, dtype, 1, runs=7, inner=3)
            decoder_speed(name, dtype, 8, runs=5, inner=1)
        say("(c) one convolution launch against F.conv2d, device events, ms per launch")
        conv_speed(256, 128, runs=7, inner=5)
        conv_speed(32, 512, runs=7, inner=20)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
