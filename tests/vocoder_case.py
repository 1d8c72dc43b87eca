"""The vocoder tests' shared cases and their float64 restatement (tests/test_vocoder_cpu.py, tests/test_vocoder_gpu.py,
tools/vocoder_bench.py).  TEST INFRASTRUCTURE: plain torch on the reference's layouts ([C, L] per utterance), nothing of the kernels.

Exact cases: inputs, biases, residuals are integers in [-2, 2], a weight has at most NZ entries of +-1 per output channel (anywhere
over its taps and input channels), the slope is 0.5 or 1 and the scale 0.5 or 1.  Every product is then a multiple of 1/2 and every
partial sum, whatever its order, a multiple of 1/2 of magnitude <= 2 NZ + 6 = 30: exact in fp32; the result, a multiple of 1/4 of magnitude
<= 30, has at most 7 significant bits: exact in bf16 and fp16.  The CPU suite checks that on the restatement alone."""
import torch
import torch.nn.functional as F

NZ = 12
TINY = dict(upsample_initial_channel=64, upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], resblock_kernel_sizes=[3, 7],
            resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5]])
V1 = dict(upsample_initial_channel=512, upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], resblock_kernel_sizes=[3, 7, 11],
          resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]])


def conv_cases(tile):
    """[(id, Cin, Cout, k, d, L, lens, slope, epilogue)]; tile(Cin, Cout, k, d): the kernel's rows per workgroup.  epilogue: a subset
    of "res", "accum", "scale"."""
    cases = [(f"k{k}d{d}", 32, 32, k, d, 70, (70, 41), 0.5, ()) for k in (3, 7, 11) for d in (1, 3, 5)]
    cases += [("c64", 64, 64, 3, 1, 40, (33, 40), 1.0, ()), ("c80to32", 80, 32, 7, 1, 40, (40, 9), 0.5, ()),
              ("c32to64", 32, 64, 7, 3, 40, (1, 40), 0.5, ()), ("len0", 32, 32, 7, 3, 9, (5, 0, 9), 0.5, ()),
              ("res", 32, 32, 3, 1, 40, (40, 17), 0.5, ("res",)), ("accum", 32, 32, 3, 1, 40, (40, 17), 0.5, ("accum",)),
              ("scale", 32, 32, 3, 1, 40, (40, 17), 1.0, ("scale",)), ("all", 64, 64, 11, 5, 40, (22, 40), 0.5, ("res", "accum", "scale"))]
    for C, k, d in ((32, 11, 5), (64, 7, 3)):
        t = tile(C, C, k, d)
        cases += [(f"c{C}L{L}", C, C, k, d, L, (L, L - 2), 0.5, ()) for L in (3, t - 1, t, t + 1)]
    return cases


UP_CASES = [(f"u{u}L{L}", 32, 16, u, L, (L, L - 1)) for u in (8, 2) for L in (1, 5)]


def ints(gen, *shape, hi=2):
    return torch.randint(-hi, hi + 1, shape, generator=gen).double()


def sparse_weight(gen, shape, out_dim=0, nz=NZ):
    """A weight of `shape` with +-1 at nz random places of every output channel's slice (dimension out_dim), zeros elsewhere."""
    moved = [shape[out_dim]] + [s for i, s in enumerate(shape) if i != out_dim]
    per = torch.zeros(moved[0], moved[1] * moved[2], dtype=torch.float64)
    for co in range(moved[0]):
        idx = torch.randperm(per.shape[1], generator=gen)[:nz]
        per[co, idx] = torch.randint(0, 2, (nz,), generator=gen).double() * 2 - 1
    return per.reshape(moved).movedim(0, out_dim).contiguous()


def lrelu(x, slope):
    return torch.where(x > 0, x, x * slope)


def conv(x, w, b, d=1, slope=1.0):
    """One utterance: x [L, Cin], the Conv1d weight [Cout, Cin, k] -> [L, Cout]."""
    return F.conv1d(lrelu(x, slope).t()[None], w, b, padding=d * (w.shape[2] - 1) // 2, dilation=d)[0].t()


def upsample(x, wt, b, u, slope=1.0):
    """One utterance: x [L, Cin], the ConvTranspose1d weight [Cin, Cout, 2u] -> [L u, Cout]."""
    return F.conv_transpose1d(lrelu(x, slope).t()[None], wt, b, stride=u, padding=u // 2)[0].t()


def ragged(fn, x, lens, *more):
    """fn on every utterance x[b, :lens[b]] (and the same rows of `more`) alone; zeros past its end."""
    rows = [fn(x[b, :l], *(m[b, :l] for m in more)) if l else None for b, l in enumerate(lens)]
    width, per = next(r for r in rows if r is not None).shape[1], max(r.shape[0] // l for r, l in zip(rows, lens) if l)
    out = torch.zeros(x.shape[0], x.shape[1] * per, width, dtype=x.dtype, device=x.device)
    for b, r in enumerate(rows):
        if r is not None:
            out[b, :r.shape[0]] = r
    return out


def _padded(gen, lens, L, C):
    """Integer rows [B, L, C]; rows past a sample's end hold 3s, which nothing may read."""
    x = ints(gen, len(lens), L, C)
    for b, l in enumerate(lens):
        x[b, l:] = 3.0
    return x


def exact_conv(case, seed=0):
    """The float64 tensors of an exact convolution case and `want` [B, L, Cout], the utterances convolved one at a time."""
    _, Cin, Cout, k, d, L, lens, slope, epi = case
    gen = torch.Generator().manual_seed(seed)
    t = dict(x=_padded(gen, lens, L, Cin), w=sparse_weight(gen, (Cout, Cin, k)), b=ints(gen, Cout), slope=slope, d=d, lens=lens,
             res=_padded(gen, lens, L, Cout) if "res" in epi else None, y0=_padded(gen, lens, L, Cout) if "accum" in epi else None,
             scale=0.5 if "scale" in epi else 1.0)
    extra = [m for m in (t["res"], t["y0"]) if m is not None]
    t["want"] = ragged(lambda x, *m: (conv(x, t["w"], t["b"], d, slope) + sum(m)) * t["scale"], t["x"], lens, *extra)
    return t


def exact_upsample(case, seed=0):
    _, Cin, Cout, u, L, lens = case
    gen = torch.Generator().manual_seed(seed)
    t = dict(x=_padded(gen, lens, L, Cin), wt=sparse_weight(gen, (Cin, Cout, 2 * u), out_dim=1), b=ints(gen, Cout), u=u, lens=lens)
    t["want"] = ragged(lambda x: upsample(x, t["wt"], t["b"], u, 0.5), t["x"], lens)
    return t


def generator_state(cfg, seed=0):
    """A reference-keyed state dict (plain `weight` keys) of N(0, 1 / fan_in) weights: activations stay O(1) through the stack."""
    gen, state, c0 = torch.Generator().manual_seed(seed), {}, cfg["upsample_initial_channel"]

    def put(name, *shape, fan):
        state[name + ".weight"] = torch.randn(*shape, generator=gen) / fan ** 0.5
        state[name + ".bias"] = torch.randn(shape[1] if name.startswith("ups") else shape[0], generator=gen) * 0.1
    put("conv_pre", c0, 80, 7, fan=80 * 7)
    nk = len(cfg["resblock_kernel_sizes"])
    for i, u in enumerate(cfg["upsample_rates"]):
        ch = c0 // 2 ** (i + 1)
        put(f"ups.{i}", 2 * ch, ch, 2 * u, fan=2 * ch * 2)
        for j, (k, ds) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            for m in range(len(ds)):
                put(f"resblocks.{i * nk + j}.convs1.{m}", ch, ch, k, fan=ch * k)
                put(f"resblocks.{i * nk + j}.convs2.{m}", ch, ch, k, fan=4 * ch * k)
    put("conv_post", 1, ch, 7, fan=ch * 7)
    return state


def generator(state, cfg, x):
    """module/hifigan.py:146-162 on x [B, 80, T] in x's dtype on x's device: float64 on the CPU is the reference of the tests, a 16-bit
    dtype on the GPU is torch's device composite (the comparison arm of the parity bound and of the benchmark)."""
    p = lambda name: (state[name + ".weight"].to(x), state[name + ".bias"].to(x))      # noqa: E731
    nk = len(cfg["resblock_kernel_sizes"])
    x = F.conv1d(x, *p("conv_pre"), padding=3)
    for i, u in enumerate(cfg["upsample_rates"]):
        x = F.conv_transpose1d(F.leaky_relu(x, 0.1), *p(f"ups.{i}"), stride=u, padding=u // 2)
        xs = None
        for j, (k, ds) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            r = x
            for m, d in enumerate(ds):
                xt = F.conv1d(F.leaky_relu(r, 0.1), *p(f"resblocks.{i * nk + j}.convs1.{m}"), padding=d * (k - 1) // 2, dilation=d)
                r = F.conv1d(F.leaky_relu(xt, 0.1), *p(f"resblocks.{i * nk + j}.convs2.{m}"), padding=(k - 1) // 2) + r
            xs = r if xs is None else xs + r
        x = xs / nk
    return torch.tanh(F.conv1d(F.leaky_relu(x), *p("conv_post"), padding=3))


def rel(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm())
