"""Motion-diffusion measurements on the GPU, at B = 32, T = 196 frames, Dd = 138 (22 joints), max_data_dim = 512, D = 768, bf16:
  (a) ofa_diffusion_q_sample (csrc/diffusion.hip) against torch's device composite of the same arithmetic: add_noise, the in-betweening
      mix, the zero padding to 512 columns and the cast;
  (b) ofa_film_fwd + ofa_film_bwd (ops.film, forward + backward) against torch's composite: the gather of the (scale | shift) rows per
      position, (scale + 1) * h + shift, and autograd's backward;
  (c) ofa_diffusion_loss forward + gradient (ops.diffusion_loss) against torch's composite: the slice of the prediction, the weighted L1
      loss, the masked per-sentence mean, and backward;
  (d) one train step of an arch-`base` model on a [TEXT 32 tokens] -> [MOTION:...,adaptor=motion_6d] micro-batch, eager and replayed
      from the captured graph (every step draws its own noise and levels on the device).
Times are device events around `inner` back-to-back calls after a warm-up, the two arms alternated in one process, median / min / max
over the runs.  Writes what it prints to profiles/diffusion_bench.txt (--out).  Usage: python tools/diffusion_bench.py"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

LINES = []
B, T, DD, W, D = 32, 196, 138, 512, 768
N_LEVELS = 1000


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


def data(dev):
    gen = torch.Generator().manual_seed(3)
    lengths = torch.randint(T // 2, T + 1, (B,), generator=gen)
    lengths[0] = T
    masks = torch.arange(T)[None, :] >= lengths[:, None]
    x0 = torch.randn(B, T, DD, generator=gen).masked_fill(masks[:, :, None], 0.0)
    noise = torch.randn(B, T, DD, generator=gen)
    t = torch.randint(0, N_LEVELS, (B,), generator=gen)
    known_w = (torch.rand(B, T, generator=gen) < 0.2).float().masked_fill(masks, 0.0)
    return [v.to(dev) for v in (x0, noise, t, masks, known_w, lengths)] + [gen]


def q_sample_bench(dev, sched):
    from ofasys_amd import ops
    x0, noise, t, masks, known_w, lengths, _ = data(dev)
    tab = sched.on(dev)

    def ours():
        return ops.diffusion_q_sample(x0, noise, t, sched, W, torch.bfloat16, known_w=known_w, masks=masks)

    def theirs():
        xt = tab.sqrt_acp[t].view(-1, 1, 1) * x0 + tab.sqrt_1m_acp[t].view(-1, 1, 1) * noise
        kw = known_w.unsqueeze(-1)
        v = (kw * x0 + (1.0 - kw) * xt).masked_fill(masks.unsqueeze(-1), 0.0)
        return torch.nn.functional.pad(v, (0, W - DD)).to(torch.bfloat16)

    diff = float((ours().float() - theirs().float()).abs().max())
    say(f"(a) ofa_diffusion_q_sample, [B, T, Dd] = [{B}, {T}, {DD}] fp32 -> [{B}, {T}, {W}] bf16, known_w and masks given; lengths "
        f"{int(lengths.min())} .. {int(lengths.max())}; 7 alternated runs of 20 calls, device events; largest difference {diff:.3g}")
    compare({"ours": "csrc/diffusion.hip, 1 launch                 ", "torch": "torch add_noise + mix + mask + pad + cast    "}, ours, theirs)


def film_bench(dev):
    from ofasys_amd import ops
    _, _, t, masks, known_w, _, gen = data(dev)
    h0 = torch.randn(B, T, D, generator=gen).to(dev).to(torch.bfloat16)
    dout = torch.randn(B, T, D, generator=gen).to(dev).to(torch.bfloat16)
    rows0 = (0.5 * torch.randn(B + 1, 2 * D, generator=gen)).to(dev).to(torch.bfloat16)
    own = torch.arange(B, device=dev, dtype=torch.int32).unsqueeze(1)
    row_of = torch.where(known_w < 0.5, own, own.new_full((), B)).contiguous()
    idx = row_of.long()

    def ours():
        h, rows = h0.detach().requires_grad_(True), rows0.detach().requires_grad_(True)
        ops.film(h, rows, row_of).backward(dout)
        return h.grad, rows.grad

    def theirs():
        h, rows = h0.detach().requires_grad_(True), rows0.detach().requires_grad_(True)
        scale, shift = rows[idx].chunk(2, dim=-1)
        ((scale + 1.0) * h + shift).backward(dout)
        return h.grad, rows.grad

    (gh, gr), (th, tr_) = ours(), theirs()
    say(f"(b) FiLM (ofa_film_fwd + ofa_film_bwd), h [{B}, {T}, {D}] bf16, rows [{B + 1}, {2 * D}], row_of given ({int((row_of == B).sum())} "
        f"positions on the shared level-0 row); forward + backward, 7 alternated runs of 20 calls, device events; largest difference: "
        f"dh {float((gh.float() - th.float()).abs().max()):.3g}, drows {float((gr.float() - tr_.float()).abs().max()):.3g} "
        "(torch sums the rows' gradient in bf16 index_put order)")
    compare({"ours": "csrc/diffusion.hip, 3 launches               ", "torch": "torch gather + fused multiply-add, backward  "}, ours, theirs)


def loss_bench(dev, sched):
    from ofasys_amd import ops
    x0, _, t, masks, _, lengths, gen = data(dev)
    pred0 = torch.randn(B, T, W, generator=gen).to(dev)
    pred0[..., :DD] = x0 + 0.5 * pred0[..., :DD]
    pred0 = pred0.to(torch.bfloat16)
    seed = torch.ones((), dtype=torch.float32, device=dev)
    w = sched.on(dev).w
    keep = (~masks).float()

    def ours():
        p = pred0.detach().requires_grad_(True)
        loss = ops.diffusion_loss(p, x0, t, sched, masks=masks, seed=seed)
        loss.backward(seed)
        return loss.detach(), p.grad

    def theirs():
        p = pred0.detach().requires_grad_(True)
        wb = w[t].view(-1, 1, 1)
        losses = (wb * p[..., :DD].float() - wb * x0).abs().mean(dim=-1)
        loss = ((keep * losses).sum(-1) / keep.sum(-1)).mean()
        loss.backward()
        return loss.detach(), p.grad

    (lo, go), (lt, gt) = ours(), theirs()
    say(f"(c) ofa_diffusion_loss, pred [{B}, {T}, {W}] bf16 read at {DD} columns, target fp32, masks given, objective `sample`; forward + "
        f"gradient, 7 alternated runs of 20 calls, device events; loss: csrc/diffusion.hip {float(lo):.6f}, torch {float(lt):.6f}; largest "
        f"gradient difference {float((go.float() - gt.float()).abs().max()):.3g}")
    compare({"ours": "csrc/diffusion.hip, 2 launches               ", "torch": "torch slice + weighted l1 + masked mean, bwd "}, ours, theirs)


def step_bench(dev, sched):
    from oracle.cases import VOCAB_EXTRA
    from ofasys_amd import Dictionary, GeneralistModel, ModalityType, Slot, ops
    from ofasys_amd.trainer import TrainStep
    x0, _, _, masks, _, lengths, gen = data(dev)
    say(f"(d) train step, arch base, [TEXT 32 tokens] -> [MOTION:...,adaptor=motion_6d], B = {B}, T = {T}, Dd = {DD}, bf16, noise and levels "
        "drawn on the device every step; 5 runs of 10 steps, device events")
    for name, use_graph in (("eager                         ", False), ("replayed from a captured graph", True)):
        d = Dictionary()
        for i in range(VOCAB_EXTRA):
            d.add_symbol(f"<text>_{i}")
        torch.manual_seed(1)
        m = GeneralistModel()
        m.cfg.arch = "base"
        m.__init__(m.cfg)
        m.cfg.adaptor.text.is_active = m.cfg.adaptor.motion_6d.is_active = True
        m.initialize(d)
        m = m.to(dev).to(torch.bfloat16)
        ops.manual_seed(1234)
        tr = TrainStep(m, lr=1e-4, clip_norm=1.0, use_graph=use_graph, graph_warmup=1)
        src = torch.randint(4, len(d), (B, 32), generator=gen).to(dev)
        value = {"value": x0, "masks": masks}
        value["value_0"] = value["value"]
        sample = {"slots": [Slot(ModalityType.TEXT, True, src), Slot(ModalityType.MOTION, False, value, attributes=["adaptor=motion_6d"])],
                  "diffusion": sched, "task": "t2m"}
        for _ in range(3):
            tr.train_step([sample])
        v = [timed(lambda: tr.train_step([sample]), 10) for _ in range(5)]
        say(f"    {name}: median {statistics.median(v) / 1e3:8.3f} ms / step (min {min(v) / 1e3:.3f}, max {max(v) / 1e3:.3f}); "
            f"main_loss {float(tr.last['main_loss']):.4f}; captured graphs {tr.captured_graphs()}")
        del tr, m
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffusion_bench.txt"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/diffusion_bench.py needs a GPU: there is no fallback")
    from ofasys_amd.diffusion import NoiseSchedule
    dev = torch.device("cuda")
    sched = NoiseSchedule(num_train_timesteps=N_LEVELS)
    say("tools/diffusion_bench.py -- motion diffusion: the three passes of csrc/diffusion.hip against torch's device composites, and a train step")
    say(f"source_id {bench.source_id()}")
    q_sample_bench(dev, sched)
    film_bench(dev)
    loss_bench(dev, sched)
    step_bench(dev, sched)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
