"""Autoregressive speech generation on the GPU: an arch-`base` model (the cfg-2 size: D = 768, 6 + 6 layers) with `text` + `audio_fbank`
active, bf16, [TEXT 64 tokens] -> [AUDIO:fbank], B = 32, 200 steps with a threshold that finishes nobody (the work is fixed):
  (a) one captured step, replayed: the step's graph with the fused kernel (csrc/speech_step.hip) against the same step with
      fused_step=False -- the unfused composition of the existing kernels, the baseline; both arms in this process, alternated;
  (b) the step's policy alone, replayed from a captured graph of its own: ofa_speech_step against the launches it replaces;
  (c) whole generate() calls: frames per second with captured steps; for scale the eager loops, and the unfused eager loop with a
      host read of the finished count every step (the reference's `finished.sum().item()`);
  (d) what a captured step costs: device memory (driver-level free memory before and after recording the 200 steps) and recording time.
Times are device events around back-to-back replays after a warm-up (a, b) or a host clock around calls that end in a synchronise (c),
median / min / max over the runs.  Writes what it prints to profiles/speech_gen_bench.txt (--out).  Usage: python tools/speech_gen_bench.py"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

LINES = []
B, S, STEPS = 32, 64, 200


def say(s):
    print(s, flush=True)
    LINES.append(s)


def stats(v, unit, scale=1.0):
    return f"median {statistics.median(v) * scale:9.3f} {unit} (min {min(v) * scale:.3f}, max {max(v) * scale:.3f})"


def build(device):
    from ofasys_amd import Dictionary, GeneralistModel
    d = Dictionary()
    for i in range(bench.V_TEXT):
        d.add_symbol(f"<text>_{i}")
    torch.manual_seed(1)
    m = GeneralistModel()
    m.cfg.arch = "base"
    m.__init__(m.cfg)
    for name in ("text", "audio_fbank"):
        getattr(m.cfg.adaptor, name).is_active = True
    m.initialize(d)
    return m.to(device).to(torch.bfloat16).eval(), d


def sample(d, device):
    from ofasys_amd import ModalityType, Slot
    g = torch.Generator().manual_seed(2)
    tokens = torch.randint(4, len(d), (B, S), generator=g).to(device)
    return {"net_input": {"slots": [Slot(ModalityType.TEXT, True, tokens), Slot(ModalityType.AUDIO, False, None)]}}


def replay_steps(gen):
    graphs = [g for _, (g, _) in sorted(gen._dec._graphs.items(), key=lambda kv: kv[0][0])]
    assert len(graphs) == STEPS
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for g in graphs:
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speech_gen_bench.txt"))
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    from ofasys_amd import AutoRegressiveSpeechGenerator, ops
    dev = torch.device("cuda:0")
    model, d = build(dev)
    smp = sample(d, dev)
    ad = model.decoder.adaptor.audio_fbank
    say("tools/speech_gen_bench.py -- autoregressive speech generation: the fused step kernel against the unfused composition")
    say(f"source_id {bench.source_id()}")
    say(f"arch base (D = 768), text + audio_fbank, bf16, [TEXT {S}] -> [AUDIO:fbank], B = {B}, {STEPS} steps, nobody finishes; prenet "
        f"{len(ad.prenet[0].layers)} x {ad.cfg.prenet_dim}, dropout {ad.prenet[0].dropout}, out_dim {ad.out_dim}")
    mk = lambda **kw: AutoRegressiveSpeechGenerator(d, max_iter=STEPS, eos_prob_threshold=2.0, graph_cap=None, **kw)     # noqa: E731
    fused, unfused = mk(), mk(fused_step=False)

    # (d) and the warm-up of (a): the first call runs eagerly, the second records the 200 steps
    cost = {}
    for name, gen in (("fused", fused), ("unfused", unfused)):
        gen.generate(model, smp)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        t = wall(lambda: gen.generate(model, smp))
        cost[name] = ((free0 - torch.cuda.mem_get_info()[0]) / STEPS / 2 ** 20, t / STEPS * 1e3)
        assert gen.fused is (name == "fused") and len(gen._dec._graphs) == STEPS
    say(f"(a) one captured step (decoder + policy), {STEPS} step graphs replayed back to back, {args.runs} alternated runs, device events")
    res = {"fused": [], "unfused": []}
    for gen in (fused, unfused):
        replay_steps(gen)
    for _ in range(args.runs):
        res["fused"].append(replay_steps(fused))
        res["unfused"].append(replay_steps(unfused))
    say(f"    fused step kernel (1 launch)        : {stats(res['fused'], 'ms / step')}")
    say(f"    unfused composition (the baseline)  : {stats(res['unfused'], 'ms / step')}")
    say(f"    fused / unfused = {statistics.median(res['fused']) / statistics.median(res['unfused']):.3f} (medians)")

    say("(b) the step's policy alone at the same shapes, each arm replayed from a captured graph of its own, 50 replays per run")
    head, prenet, proj = ad.step_weights()
    x = torch.randn(B, 768, device=dev).to(torch.bfloat16)
    alone = {}
    for name, flag in (("fused", True), ("unfused", False)):
        st = {k: v.clone() for k, v in fused._dec.state.items() if k != "host"}
        with torch.no_grad():
            ops.speech_step(x, head, prenet, proj, st, 0, 0.5, fused=flag)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.no_grad(), torch.cuda.graph(g):
            ops.speech_step(x, head, prenet, proj, st, 0, 0.5, fused=flag)
            ops.rng_advance()
        alone[name] = (g, st)
    res = {"fused": [], "unfused": []}
    for _ in range(args.runs + 1):
        for name, (g, _) in alone.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e3 / 50)
    for name in res:
        res[name] = res[name][1:]
    say(f"    ofa_speech_step + the stream-position add : {stats(res['fused'], 'us')}")
    say(f"    the launches it replaces                 : {stats(res['unfused'], 'us')}")

    say(f"(c) whole generate() calls ({STEPS} steps, encoder, postnet and the copy to the host included), {args.runs} runs, host clock")
    frames = B * ad.n_frames_per_step * STEPS

    class HostRead:
        """The reference's loop shape: the unfused policy, eagerly, and a host read of the finished count after every step."""

        def __init__(self):
            self.gen = mk(fused_step=False, use_graph=False)
            self.orig = ops.speech_step

        def __call__(self):
            def with_read(x, head, prenet, proj, state, step, p_drop, fused=True):
                self.orig(x, head, prenet, proj, state, step, p_drop, fused=fused)
                state["nfin"].item()
            ops.speech_step = with_read
            try:
                self.gen.generate(model, smp)
            finally:
                ops.speech_step = self.orig

    arms = [("captured steps, fused kernel", lambda: fused.generate(model, smp)),
            ("captured steps, unfused", lambda: unfused.generate(model, smp)),
            ("eager steps, fused kernel", (lambda g: lambda: g.generate(model, smp))(mk(use_graph=False))),
            ("eager steps, unfused", (lambda g: lambda: g.generate(model, smp))(mk(use_graph=False, fused_step=False))),
            ("eager, unfused, host read per step", HostRead())]
    for name, fn in arms:
        fn()
        v = [wall(fn) for _ in range(args.runs)]
        say(f"    {name:36s}: {stats(v, 'ms / call', 1e3)}; {frames / statistics.median(v):9.0f} frames / s")
    say(f"(d) recording the {STEPS} steps (one hipGraph per step length; the second generate() call)")
    for name, (mb, ms) in cost.items():
        say(f"    {name:8s}: {mb:7.3f} MiB of device memory per recorded step (driver-level free memory), {ms:7.2f} ms per step to record and run once")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
