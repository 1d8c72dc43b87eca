"""Motion-generation measurements on the GPU, at B = 32, T = 196 frames, Dd = 138 (22 joints), max_data_dim = 512, bf16:
  (a) ofa_diffusion_sample_step (csrc/diffusion_step.hip), in-betweening with masks, against torch's device composite of the same chain:
      the slice of the prediction, the rectification, the dense interp_w matmul and the mix, the scheduler step, the adaptor's mix, the
      zero padding to 512 columns and the cast;
  (b) one sampling step of an arch-`base` model on [TEXT 32 tokens] -> [MOTION:...,adaptor=motion_6d], 50 DDIM steps: the eager loop
      against the captured step, ms per step over whole generate() calls;
  (c) what caching the cross-attention K / V of the static encoder output would save: the decoder layers' k / v projections of the
      encoder output, timed alone, per step.
Times are device events around `inner` back-to-back calls after a warm-up, the two arms alternated in one process, median / min / max
over the runs.  Writes what it prints to profiles/motion_gen_bench.txt (--out).  Usage: python tools/motion_gen_bench.py"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

LINES = []
B, T, DD, W = 32, 196, 138, 512
N_STEPS = 50


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def say(s):
    print(s, flush=True)
    LINES.append(s)


def spread(v, scale=1.0):
    return f"median {statistics.median(v) / scale:8.3f} (min {min(v) / scale:.3f}, max {max(v) / scale:.3f})"


def batch(dev):
    from ofasys_amd.preprocessor.motion import interpolate_weight
    gen = torch.Generator().manual_seed(3)
    lengths = torch.randint(T // 2, T + 1, (B,), generator=gen)
    lengths[0] = T
    masks = torch.arange(T)[None, :] >= lengths[:, None]
    known_w = (torch.rand(B, T, generator=gen) < 0.2).float().masked_fill(masks, 0.0)
    known_w[:, 3] = 1.0
    interp_w = torch.stack([torch.nn.functional.pad(interpolate_weight(k[:n]), (0, T - n, 0, T - n)) for k, n in zip(known_w, lengths.tolist())])
    value_0 = torch.randn(B, T, DD, generator=gen).masked_fill(masks[:, :, None], 0.0)
    return [v.to(dev) for v in (masks, known_w, interp_w, value_0)] + [lengths, gen]


def kernel_bench(dev, sched):
    from ofasys_amd import ops
    masks, known_w, interp_w, value_0, lengths, gen = batch(dev)
    plan = sched.sampling_on(dev)
    pred = torch.randn(B, T, W, generator=gen).to(dev).to(torch.bfloat16)
    x_t0 = torch.randn(B, T, DD, generator=gen).to(dev)
    nbr, nbw = ops.diffusion_neighbours(interp_w)
    st = {"x_t": x_t0.clone(), "img": torch.zeros_like(x_t0), "xin": torch.zeros(B, T, W, dtype=torch.bfloat16, device=dev),
          "level": torch.zeros(B, dtype=torch.int64, device=dev), "counter": torch.zeros(2, dtype=torch.int32, device=dev),
          "coef": plan.coef, "timesteps": plan.timesteps, "masks": masks, "value_0": value_0, "known_w": known_w, "nbr": nbr, "nbw": nbw}
    s = 20
    c0, c1, _ = [float(c) for c in plan.coef[s]]
    kw, keep = known_w.unsqueeze(-1), (~masks).unsqueeze(-1)

    def ours():
        st["counter"][0] = s                                      # (a fill kernel: both arms pay one small launch for the step index)
        ops.diffusion_sample_step(pred, st)
        return st["img"], st["xin"]

    def theirs():
        level = plan.timesteps[s + 1].expand(B)                    # noqa: F841  (the level of the next call)
        x = pred[..., :DD].float()
        a = x[..., 6:].reshape(B, T, -1, 6)
        b1 = torch.nn.functional.normalize(a[..., :3], dim=-1)
        b2 = torch.nn.functional.normalize(a[..., 3:] - (b1 * a[..., 3:]).sum(-1, keepdim=True) * b1, dim=-1)
        x = torch.cat((x[..., :6], torch.cat((b1, b2), -1).reshape(B, T, -1)), -1)
        x = x + torch.matmul(interp_w, value_0 - x)
        img = (kw * value_0 + (1.0 - kw) * x) * keep
        x_t = (c0 * img + c1 * x_t0) * keep
        xin = torch.nn.functional.pad((kw * value_0 + (1.0 - kw) * x_t) * keep, (0, W - DD)).to(torch.bfloat16)
        return img, xin

    st["x_t"].copy_(x_t0)
    (io, xo), (it, xt) = ours(), theirs()
    say(f"(a) ofa_diffusion_sample_step, pred [{B}, {T}, {W}] bf16 read at {DD} columns, in-betweening ({int(known_w.sum())} known frames) and "
        f"masks (lengths {int(lengths.min())} .. {int(lengths.max())}), a DDIM middle step; 7 alternated runs of 20 calls, device events, us per "
        f"call; largest difference: img {float((io - it).abs().max()):.3g}, denoiser input {float((xo.float() - xt.float()).abs().max()):.3g}")
    for fn in (ours, theirs):
        timed(fn, 5)
    res = {"ours": [], "torch": []}
    for _ in range(7):
        res["ours"].append(timed(ours, 20))
        res["torch"].append(timed(theirs, 20))
    say(f"    csrc/diffusion_step.hip, 1 launch (+ the index fill)   : {spread(res['ours'])} us")
    say(f"    torch composite with the dense [B, T, T] interp_w matmul: {spread(res['torch'])} us")
    say(f"    kernel / torch = {statistics.median(res['ours']) / statistics.median(res['torch']):.3f} (medians; both include the host's launch work)")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.diffusion_sample_step(pred, st)
    timed(g.replay, 5)
    say(f"    the launch replayed from a captured graph              : {spread([timed(g.replay, 20) for _ in range(7)])} us")


def model_bench(dev):
    from oracle.cases import VOCAB_EXTRA
    from ofasys_amd import Dictionary, DiffusionGenerator, GeneralistModel, ModalityType, Slot
    masks, known_w, interp_w, value_0, lengths, gen = batch(dev)
    d = Dictionary()
    for i in range(VOCAB_EXTRA):
        d.add_symbol(f"<text>_{i}")
    torch.manual_seed(1)
    m = GeneralistModel()
    m.cfg.arch = "base"
    m.__init__(m.cfg)
    m.cfg.adaptor.text.is_active = m.cfg.adaptor.motion_6d.is_active = True
    m.initialize(d)
    m = m.to(dev).to(torch.bfloat16).eval()
    src = torch.randint(4, len(d), (B, 32), generator=gen).to(dev)
    value = {"value": value_0, "masks": masks, "known_w": known_w, "interp_w": interp_w, "value_0": value_0}
    sample = {"net_input": {"slots": [Slot(ModalityType.TEXT, True, src), Slot(ModalityType.MOTION, False, value, attributes=["adaptor=motion_6d"])]}}
    args = {"scheduler": "DDIMScheduler", "num_train_timesteps": 1000, "num_inference_steps": N_STEPS}
    say(f"(b) DiffusionGenerator.generate, arch base, [TEXT 32 tokens] -> [MOTION:...,adaptor=motion_6d], B = {B}, T = {T}, Dd = {DD}, bf16, "
        f"in-betweening, {N_STEPS} DDIM steps; 5 alternated runs of one generate() each after a warm-up of two, device events, ms per step "
        "(the encoder, the first launch and the copy of the result to the host included)")
    gens = {"eager": DiffusionGenerator(None, args, use_graph=False), "graph": DiffusionGenerator(None, args, use_graph=True)}
    res = {k: [] for k in gens}
    for k, g in gens.items():
        for _ in range(2):
            g.generate(m, sample)
    for _ in range(5):
        for k, g in gens.items():
            res[k].append(timed(lambda: g.generate(m, sample), 1) / N_STEPS)
    say(f"    eager loop                    : {spread(res['eager'], 1e3)} ms / step")
    say(f"    one captured step, replayed   : {spread(res['graph'], 1e3)} ms / step; captured graphs {gens['graph'].captures}")
    say(f"    captured / eager = {statistics.median(res['graph']) / statistics.median(res['eager']):.3f} (medians)")
    # (c) the k | v projections of the static encoder output, which every step repeats
    with torch.no_grad():
        enc = m.encoder(sample["net_input"]["slots"][:1])["encoder_out"][0]
        layers = [l.encoder_attn for l in m.decoder.layers]

        def kv():
            return [(a.k_proj(enc), a.v_proj(enc)) for a in layers]

        timed(kv, 5)
        v = [timed(kv, 20) for _ in range(7)]
    say(f"(c) NOT BUILT, future work: the {len(layers)} decoder layers' k_proj / v_proj of the static encoder output [{enc.shape[0]}, {B}, {enc.shape[2]}], "
        f"which every step repeats and a cross-attention cache over the steps would run once per batch; 7 runs of 20 calls, eager: {spread(v)} us per "
        "step (an upper bound of the saving: the captured step pays no launch work for them)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_gen_bench.txt"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/motion_gen_bench.py needs a GPU: there is no fallback")
    from ofasys_amd.diffusion import NoiseSchedule
    dev = torch.device("cuda")
    say("tools/motion_gen_bench.py -- motion generation: the sampling step of csrc/diffusion_step.hip against torch's device composite, and the sampling loop")
    say(f"source_id {bench.source_id()}")
    kernel_bench(dev, NoiseSchedule(num_train_timesteps=1000, num_inference_steps=N_STEPS))
    model_bench(dev)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
