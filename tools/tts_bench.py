"""Text-to-speech measurements on the GPU, at B = 32, T = 800 frames, F = 80, bf16:
  (a) ofa_tacotron2_loss forward + gradient (csrc/tacotron_loss.hip through ops.tacotron2_loss) against torch's device composite on the SAME
      tensors: masked l1_loss + mse_loss twice + binary_cross_entropy_with_logits, and backward;
  (b) the postnet (5 layers, 512 channels, k = 5, dropout 0.5, train mode) forward + backward through the kernels (time-unfold, MFMA GEMM with
      the column-statistics epilogue, BatchNorm, tanh + dropout) against the same module's nn.Conv1d / nn.BatchNorm1d / nn.Tanh / nn.Dropout
      run by torch on the device;
  (c) one train step of an arch-`tiny` model on a [TEXT] -> [AUDIO:fbank] micro-batch (64 source tokens), eager and replayed from the
      captured graph.  (A pack plan with an fbank target is refused, so the step runs on the padded layout.)
  --count: instead, the host-side launch census of ONE eager caption-only train step (no text-to-speech micro-batch): C-ABI calls and
      torch operator calls.  The tool runs unchanged on an older tree (it needs nothing of the text-to-speech code for this), so the two
      censuses can be compared.
Times are device events around `inner` back-to-back calls after a warm-up, the two arms alternated, median / min / max over the runs.
Writes what it prints to profiles/tts_bench.txt (--out).  Usage: python tools/tts_bench.py"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

LINES = []
B, T, F = 32, 800, 80


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


def compare(names, ours, theirs, runs=7, inner=20):
    for fn in (ours, theirs):
        timed(fn, 5)
    res = {"ours": [], "torch": []}
    for _ in range(runs):
        res["ours"].append(timed(ours, inner))
        res["torch"].append(timed(theirs, inner))
    for k in ("ours", "torch"):
        v = res[k]
        say(f"    {names[k]}: median {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f})")
    mo, mt = statistics.median(res["ours"]), statistics.median(res["torch"])
    say(f"    kernels / torch = {mo / mt:.2f} (medians; both include the host's launch work of an eager call)")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ours()
    timed(g.replay, 5)
    v = [timed(g.replay, inner) for _ in range(runs)]
    say(f"    kernels replayed from a captured graph: median {statistics.median(v):8.1f} us (min {min(v):.1f}, max {max(v):.1f})")


def frames(dev, dtype):
    gen = torch.Generator().manual_seed(3)
    lengths = torch.randint(T // 2, T + 1, (B,), generator=gen)
    lengths[0] = T
    tgt = torch.randn(B, T, F, generator=gen)
    tgt = tgt * (torch.arange(T)[None, :, None] < lengths[:, None, None])
    return tgt.to(dev).to(dtype), lengths.to(dev), gen


def loss_bench(dev):
    from ofasys_amd import ops
    import torch.nn.functional as Fn
    dtype = torch.bfloat16
    tgt, lengths, gen = frames(dev, dtype)
    feat = (tgt.float() + 0.5 * torch.randn(B, T, F, generator=gen).to(dev)).to(dtype)
    post = (tgt.float() + 0.25 * torch.randn(B, T, F, generator=gen).to(dev)).to(dtype)
    eos = (2 * torch.randn(B, T, 1, generator=gen)).to(dev).to(dtype)
    seed = torch.ones((), dtype=torch.float32, device=dev)
    mask = torch.arange(T, device=dev)[None, :] < lengths[:, None]
    eos_tgt = (torch.arange(T, device=dev)[None, :] == (lengths[:, None] - 1)).float()
    pw = torch.tensor(5.5, device=dev)

    def ours():
        f, p, e = (t.detach().requires_grad_(True) for t in (feat, post, eos))
        loss, _ = ops.tacotron2_loss(f, p, e, tgt, lengths, 5.5, "mean", seed=seed)
        loss.backward(seed)
        return loss.detach(), f.grad

    def theirs():
        f, p, e = (t.detach().requires_grad_(True) for t in (feat, post, eos))
        _t, _f, _p = tgt[mask].float(), f[mask].float(), p[mask].float()
        loss = (Fn.l1_loss(_f, _t) + Fn.l1_loss(_p, _t) + Fn.mse_loss(_f, _t) + Fn.mse_loss(_p, _t)
                + Fn.binary_cross_entropy_with_logits(e[mask].squeeze().float(), eos_tgt[mask], pos_weight=pw))
        loss.backward()
        return loss.detach(), f.grad

    lo, go = ours()
    lt, gt = theirs()
    say(f"(a) ofa_tacotron2_loss, B = {B}, T = {T}, F = {F}, bf16; lengths {int(lengths.min())} .. {int(lengths.max())}, "
        f"{int(lengths.sum())} valid frames; forward + gradient, 7 alternated runs of 20 calls, device events")
    say(f"    loss: csrc/tacotron_loss.hip {float(lo):.6f}, torch {float(lt):.6f}; largest gradient difference "
        f"{float((go.float() - gt.float()).abs().max()):.3g}")
    compare({"ours": "csrc/tacotron_loss.hip, 2 launches          ", "torch": "torch masked l1 + mse x2 + bce, backward    "}, ours, theirs)


def postnet_bench(dev):
    from ofasys_amd import ops
    from ofasys_amd.adaptor.audio import Postnet
    dtype = torch.bfloat16
    torch.manual_seed(5)
    net = Postnet(F, 512, 5, 5, 0.5).to(dev).to(dtype)
    net.train()
    x0, _, gen = frames(dev, dtype)
    dout = torch.randn(B, T, F, generator=gen).to(dev).to(dtype)
    ops.manual_seed(11)

    def ours():
        x = x0.detach().requires_grad_(True)
        net.zero_grad(set_to_none=True)
        net(x).backward(dout)
        return x.grad

    def theirs():
        x = x0.detach().requires_grad_(True)
        net.zero_grad(set_to_none=True)
        h = x.transpose(1, 2)
        for conv in net.convolutions:
            h = conv(h)
        h.transpose(1, 2).backward(dout)
        return x.grad

    say(f"(b) postnet, 5 layers x 512 channels, k = 5, dropout 0.5, train mode, [B, T, F] = [{B}, {T}, {F}] bf16; forward + backward, "
        "7 alternated runs of 20 calls, device events")
    compare({"ours": "unfold + MFMA GEMM + BatchNorm + tanh/dropout kernels", "torch": "nn.Conv1d / BatchNorm1d / Tanh / Dropout (torch)      "},
            ours, theirs)


def _tiny_engine(dev, use_graph, tts=True):
    from oracle.cases import VOCAB_EXTRA
    from ofasys_amd import Dictionary, GeneralistModel, ops
    from ofasys_amd.trainer import TrainStep
    d = Dictionary()
    for i in range(VOCAB_EXTRA):
        d.add_symbol(f"<text>_{i}")
    torch.manual_seed(1)
    m = GeneralistModel()
    m.cfg.arch = "tiny"
    m.__init__(m.cfg)
    m.cfg.adaptor.text.is_active = True
    if tts:
        m.cfg.adaptor.audio_fbank.is_active = True
    m.initialize(d)
    m = m.to(dev).to(torch.bfloat16)
    ops.manual_seed(1234)
    return TrainStep(m, lr=1e-4, clip_norm=1.0, use_graph=use_graph, graph_warmup=1), d


def step_bench(dev):
    from ofasys_amd import ModalityType, Slot
    tgt, lengths, gen = frames(dev, torch.bfloat16)
    prev = torch.cat((torch.zeros_like(tgt[:, :1]), tgt[:, :-1]), 1)
    say(f"(c) train step, arch tiny, [TEXT 64 tokens] -> [AUDIO:fbank], B = {B}, T = {T}, F = {F}, bf16, padded layout (a pack plan with "
        "an fbank target is refused); 5 runs of 10 steps, device events")
    for name, use_graph in (("eager                         ", False), ("replayed from a captured graph", True)):
        tr, d = _tiny_engine(dev, use_graph)
        src = torch.randint(4, len(d), (B, 64), generator=gen).to(dev)
        sample = {"slots": [Slot(ModalityType.TEXT, True, src), Slot(ModalityType.AUDIO, False, {"fbank": prev, "fbank_lengths": lengths})],
                  "target": tgt, "target_lengths": lengths, "bce_pos_weight": 1.0, "task": "tts"}
        for _ in range(3):
            tr.train_step([sample])
        v = [timed(lambda: tr.train_step([sample]), 10) for _ in range(5)]
        say(f"    {name}: median {statistics.median(v) / 1e3:8.3f} ms / step (min {min(v) / 1e3:.3f}, max {max(v) / 1e3:.3f}); "
            f"loss {float(tr.last['stats'][1]):.4f}")


def census(dev):
    """C-ABI calls and torch operator calls of one eager caption-only train step (the third: caches are warm)."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from ofasys_amd import ModalityType, Slot
    from ofasys_amd import lib as L
    tr, d = _tiny_engine(dev, False, tts=False)
    gen = torch.Generator().manual_seed(3)
    src = torch.randint(4, len(d), (8, 24), generator=gen).to(dev)
    prev = torch.randint(4, len(d), (8, 12), generator=gen)
    prev[:, 0] = 0
    target = torch.cat((prev[:, 1:], torch.full((8, 1), 2)), 1).to(dev)
    sample = {"slots": [Slot(ModalityType.TEXT, True, src), Slot(ModalityType.TEXT, False, prev.to(dev))], "target": target, "task": "caption"}
    counts = {"abi": 0, "aten": 0}
    names = {}

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            counts["aten"] += 1
            return func(*args, **(kwargs or {}))

    orig = L._Lib.call

    def call(self, name, *args):
        counts["abi"] += 1
        names[name] = names.get(name, 0) + 1
        return orig(self, name, *args)

    for _ in range(2):
        tr.train_step([sample])
    L._Lib.call = call
    try:
        with Count():
            tr.train_step([sample])
    finally:
        L._Lib.call = orig
    torch.cuda.synchronize()
    say(f"launch census of one eager caption-only train step (arch tiny, B = 8, 24 -> 12 tokens): {counts['abi']} C-ABI calls over "
        f"{len(names)} entry points, {counts['aten']} torch operator calls on the calling thread; loss {float(tr.last['stats'][1]):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tts_bench.txt"))
    ap.add_argument("--count", action="store_true")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tts_bench.py needs a GPU: there is no fallback")
    dev = torch.device("cuda")
    if opt.count:
        say(f"source_id {bench.source_id()}")
        census(dev)
        return
    say("tools/tts_bench.py -- text-to-speech: the fused Tacotron2 loss and the postnet against torch's device path, and a train step")
    say(f"source_id {bench.source_id()}")
    loss_bench(dev)
    postnet_bench(dev)
    step_bench(dev)
    census(dev)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
