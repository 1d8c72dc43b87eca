"""The image_vit hot path on the GPU, bf16, four things:
  (a) ofa_quick_gelu_fwd / ofa_quick_gelu_bwd (with the column-sum partial rows) at 6272 x 3072 -- vit_base's MLP at batch 32 -- next to
      ofa_gelu_fwd / ofa_gelu_bwd (the erf GELU: the yardstick) on the same tensors in the same run.  The yardstick is timed TWICE per
      round (before and after the QuickGELU arm); the difference of its two medians is the run-to-run spread, written next to the figures.
      QuickGELU does strictly less arithmetic on the same bytes, so it must not be slower than the yardstick by more than that spread:
      the tool says which way it came out, and exits non-zero if it is slower;
  (b) one ResidualAttentionBlock (width 768, 12 heads, 196 tokens, batch 32) forward + backward;
  (c) the vit_base backbone forward + backward at batch 32;
  each of (b), (c) next to a plain-torch device restatement of the same block written here (F.layer_norm, matmuls,
  F.scaled_dot_product_attention, x * sigmoid(1.702 x)) on the same weights.
Times are device events around `inner` back-to-back calls after a warm-up -- `inner` sized so that a timed window lasts about 0.1 s: 6000
calls for (a), 100 for (b), 12 for (c) --, the arms alternated, median / min / max over the rounds.
This is the first measurement of these paths: no earlier time is recorded anywhere, so nothing was promised and nothing is compared
with a past figure.  Writes what it prints to profiles/vit_bench.txt (--out).  Reads nothing outside the repository.
Usage: python tools/vit_bench.py"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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
    return e0.elapsed_time(e1) * 1e3 / inner


def fmt(v):
    return f"median {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f})"


def alternate(arms, rounds, inner):
    """arms: [(name, fn)] (a name may repeat: its rounds are kept per position) -> [[times] per position]."""
    for _, fn in arms:
        timed(fn, 3)
    res = [[] for _ in arms]
    for _ in range(rounds):
        for i, (_, fn) in enumerate(arms):
            res[i].append(timed(fn, inner))
    return res


def gelu_bench(dev, rows=6272, cols=3072, rounds=7, inner=6000):
    from ofasys_amd import kernels as K
    g = torch.Generator(device="cpu").manual_seed(5)
    h = (3 * torch.randn(rows, cols, generator=g)).to(torch.bfloat16).to(dev)
    dy = torch.randn(rows, cols, generator=g).to(torch.bfloat16).to(dev)
    nbytes_f, nbytes_b = 2 * h.numel() * 2, 3 * h.numel() * 2
    say(f"(a) QuickGELU next to the erf GELU, {rows} x {cols} bf16 (vit_base c_fc output, batch 32): {rounds} rounds of {inner} calls "
        f"per timed window (about 0.1 s each), device events; order per round: erf, quick, erf again; the tensors ({h.numel() * 2 / 1e6:.1f} MB "
        f"each) stay in the 256 MiB Infinity Cache between calls: warm figures")
    ok = True
    for tag, quick, erf, nb in (("forward ", lambda: K.quick_gelu_fwd(h), lambda: K.gelu_fwd(h), nbytes_f),
                                ("backward", lambda: K.quick_gelu_bwd(dy, h, want_partials=True), lambda: K.gelu_bwd(dy, h), nbytes_b)):
        e1, q, e2 = alternate([("erf", erf), ("quick", quick), ("erf", erf)], rounds, inner)
        m1, mq, m2 = statistics.median(e1), statistics.median(q), statistics.median(e2)
        spread = abs(m1 - m2)
        yard = max(m1, m2)
        say(f"    {tag} ofa_gelu (yardstick, first)   {fmt(e1)}  {nb / m1 / 1e6:6.2f} TB/s")
        say(f"    {tag} ofa_quick_gelu                {fmt(q)}  {nb / mq / 1e6:6.2f} TB/s"
            + ("  (with the fp32 partial rows of the column sums)" if tag == "backward" else ""))
        say(f"    {tag} ofa_gelu (yardstick, second)  {fmt(e2)}  {nb / m2 / 1e6:6.2f} TB/s")
        slower = mq > yard + spread
        ok = ok and not slower
        say(f"    {tag} run-to-run spread of the yardstick {spread:.1f} us; quick / yardstick = {mq / yard:.3f}: "
            + ("QuickGELU IS SLOWER than the erf GELU by more than the spread" if slower else
               "QuickGELU is not slower than the erf GELU (within the spread or faster)"))
    return ok


def torch_block(p, x, heads):
    """One pre-LN block on [B, T, D] in plain torch, same parameters."""
    B, T, D = x.shape
    n = F.layer_norm(x, (D,), p["ln_1.weight"], p["ln_1.bias"])
    q, k, v = (t.view(B, T, heads, D // heads).transpose(1, 2) for t in F.linear(n, p["attn.in_proj_weight"], p["attn.in_proj_bias"]).split(D, -1))
    a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, D)
    x = x + F.linear(a, p["attn.out_proj.weight"], p["attn.out_proj.bias"])
    n = F.layer_norm(x, (D,), p["ln_2.weight"], p["ln_2.bias"])
    hmid = F.linear(n, p["mlp.c_fc.weight"], p["mlp.c_fc.bias"])
    return x + F.linear(hmid * torch.sigmoid(1.702 * hmid), p["mlp.c_proj.weight"], p["mlp.c_proj.bias"])


def torch_backbone(m, params, img):
    p = m.patch_size
    x = F.conv2d(img, params["conv1.weight"], stride=p).flatten(2).transpose(1, 2)
    x = x + params["positional_embedding"][1:]
    x = F.layer_norm(x, (m.width,), params["ln_pre.weight"], params["ln_pre.bias"])
    heads = m.transformer.resblocks[0].attn.num_heads
    for i in range(len(m.transformer.resblocks)):
        pre = f"transformer.resblocks.{i}."
        x = torch_block({k[len(pre):]: v for k, v in params.items() if k.startswith(pre)}, x, heads)
    return x


def fwd_bwd(fn, params):
    def run():
        for q in params:
            q.grad = None
        fn().float().sum().backward()
    return run


def model_bench(dev, rounds=7):
    from ofasys_amd.module.vit import ResidualAttentionBlock, vit_base
    torch.manual_seed(0)
    B, T, D, heads = 32, 196, 768, 12
    blk = ResidualAttentionBlock(D, heads).to(dev).to(torch.bfloat16)
    x = torch.randn(B, T, D, device=dev).to(torch.bfloat16).requires_grad_(True)
    bp = dict(blk.named_parameters())
    ours, theirs = fwd_bwd(lambda: blk(x), list(bp.values()) + [x]), fwd_bwd(lambda: torch_block(bp, x, heads), list(bp.values()) + [x])
    d = float((blk(x).float() - torch_block(bp, x, heads).float()).abs().max())
    say(f"(b) one ResidualAttentionBlock, width {D}, {heads} heads, {T} tokens, batch {B}, bf16, forward + backward, eager "
        f"(both arms include the host's launch work); largest output difference between the arms {d:.3g}")
    say(f"    {rounds} rounds of {100} calls per timed window (about 0.1 s each)")
    a, b = alternate([("ours", ours), ("torch", theirs)], rounds, 100)
    say(f"    module/vit.py (HIP kernels)       {fmt(a)}")
    say(f"    plain torch on the same weights   {fmt(b)}")
    say(f"    ours / torch = {statistics.median(a) / statistics.median(b):.2f}")

    m = vit_base().to(dev).to(torch.bfloat16)
    img = torch.randn(B, 3, 224, 224, device=dev).to(torch.bfloat16)
    mp = dict(m.named_parameters())
    ours = fwd_bwd(lambda: m(img)[0], list(mp.values()))
    theirs = fwd_bwd(lambda: torch_backbone(m, mp, img), list(mp.values()))
    d = float((m(img)[0].float().view(B, T, D) - torch_backbone(m, mp, img).float()).abs().max())
    say(f"(c) the vit_base backbone (9 blocks), batch {B}, 224 x 224, bf16, forward + backward, eager; largest output difference "
        f"between the arms {d:.3g}")
    say(f"    {rounds} rounds of {12} calls per timed window (about 0.1 s each)")
    a, b = alternate([("ours", ours), ("torch", theirs)], rounds, 12)
    say(f"    module/vit.py (HIP kernels)       {fmt(a)}")
    say(f"    plain torch on the same weights   {fmt(b)}")
    say(f"    ours / torch = {statistics.median(a) / statistics.median(b):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit_bench.txt"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/vit_bench.py needs a GPU: there is no fallback")
    dev = torch.device("cuda")
    say("tools/vit_bench.py -- the image_vit backbone's hot path, bf16: QuickGELU kernels against the erf GELU kernels; one block and the "
        "vit_base backbone against a plain-torch restatement")
    say("first measurement of these paths: no earlier time is recorded, nothing was promised")
    say(f"source_id {bench.source_id()}")
    ok = gelu_bench(dev)
    model_bench(dev)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    if not ok:
        raise SystemExit("QuickGELU is slower than the erf GELU yardstick by more than its run-to-run spread (see (a))")


if __name__ == "__main__":
    main()
