"""The VQGAN decoder tests' shared cases and their float64 restatement (tests/test_vqgan_cpu.py, tests/test_vqgan_gpu.py,
tools/vqgan_bench.py).  TEST INFRASTRUCTURE: plain torch on NCHW maps, written from the formulas -- GroupNorm(32, eps 1e-6), swish
x sigmoid(x), 3 x 3 / 1 x 1 convolutions, nearest x2 interpolation, one-head bmm attention -- and nothing of the kernels.  Every function
computes in the dtype and on the device of its input: float64 on the CPU is the tests' reference, a 16-bit dtype on the GPU is torch's
device composite (the comparison arm of the 2 x bound and of the benchmark).

Exact cases: inputs in [-2, 2], weights in {-1, 0, 1} with one in eight non-zero, bias and residual in [-2, 2], all integers.  Every
product and partial sum is an integer below 2^24: exact in fp32 in any order; a result of magnitude <= 256 is exact in bf16 and fp16
(exact_conv asserts it)."""
import torch
import torch.nn.functional as F

TINY = dict(embed_dim=32, n_embed=64, ddconfig=dict(ch=32, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[8], dropout=0.0,
                                                     in_channels=3, resolution=16, z_channels=32, double_z=False))
F8 = dict(embed_dim=256, n_embed=8192, ddconfig=dict(ch=128, out_ch=3, ch_mult=(1, 1, 2, 4), num_res_blocks=2, attn_resolutions=[32], dropout=0.0,
                                                      in_channels=3, resolution=256, z_channels=256, double_z=False))


def conv_cases(plan):
    """[(id, H, W, Cin, Cout)] (H, W: the stored map's; B = 2 throughout) from plan(Cin, Cout) -> (tile, slice, channel block, lds)."""
    T = plan(32, 32)[0]
    one = 96                                                               # the largest Cin that is ONE slice
    assert plan(one, 32)[1] == one and plan(one + 32, 32)[1] < one + 32 and plan(32, 128)[2] == 128
    cases = [(f"{h}x{w}", h, w, 32, 32) for h, w in ((1, 1), (T - 1, T + 1), (T + 1, T - 1), (T // 2, T // 2 + 1))]
    cases += [(f"c{ci}to{co}", 5, 7, ci, co) for ci, co in ((one, 32), (one + 32, 32), (160, 64), (32, 96), (32, 128 + 32))]
    return cases


def ints(gen, *shape, hi=2):
    return torch.randint(-hi, hi + 1, shape, generator=gen).double()


def swish(x):
    return x * torch.sigmoid(x)


def conv3x3(x, w, b, norm=None, res=None, up=False):
    """x NCHW; norm = (gamma, beta) or None: GroupNorm + swish first; up: nearest x2 after that, before the convolution."""
    if norm is not None:
        x = swish(F.group_norm(x, 32, norm[0], norm[1], eps=1e-6))
    if up:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    y = F.conv2d(x, w, b, padding=1)
    return y if res is None else y + res


def exact_conv(case, up, seed=0):
    """The float64 tensors (NCHW, weight [Cout, Cin, 3, 3]) of an exact case and its results without and with the residual."""
    _, H, W, Cin, Cout = case
    gen, s = torch.Generator().manual_seed(seed), 2 if up else 1
    t = dict(x=ints(gen, 2, Cin, H, W), b=ints(gen, Cout), res=ints(gen, 2, Cout, H * s, W * s))
    t["w"] = ints(gen, Cout, Cin, 3, 3, hi=1) * (torch.rand(Cout, Cin, 3, 3, generator=gen) < 0.125)
    t["want"] = conv3x3(t["x"], t["w"], t["b"], up=up)
    t["want_res"] = t["want"] + t["res"]
    for v in (t["want"], t["want_res"]):
        assert torch.equal(v, v.round()) and float(v.abs().max()) <= 256, "change the seed, not the bound"
    return t


def rows(x):
    """NCHW -> contiguous NHWC rows."""
    return x.permute(0, 2, 3, 1).contiguous()


def decoder(state, dd, z, prefix="decoder."):
    """taming's Decoder on z NCHW from a reference-keyed state dict, in z's dtype on z's device."""
    p = lambda name: (state[prefix + name + ".weight"].to(z), state[prefix + name + ".bias"].to(z))      # noqa: E731

    def res(name, x):
        h = conv3x3(x, *p(name + ".conv1"), norm=p(name + ".norm1"))
        skip = F.conv2d(x, *p(name + ".nin_shortcut")) if prefix + name + ".nin_shortcut.weight" in state else x
        return conv3x3(h, *p(name + ".conv2"), norm=p(name + ".norm2"), res=skip)

    def attn(name, x):
        B, C, H, W = x.shape
        h = F.group_norm(x, 32, *p(name + ".norm"), eps=1e-6)
        q, k, v = (F.conv2d(h, *p(f"{name}.{n}")).reshape(B, C, H * W) for n in "qkv")
        a = torch.softmax(torch.bmm(q.transpose(1, 2), k) * C ** -0.5, dim=2)                            # [B, query, key]
        return x + F.conv2d(torch.bmm(v, a.transpose(1, 2)).reshape(B, C, H, W), *p(name + ".proj_out"))

    levels, res_h = len(dd["ch_mult"]), z.shape[2]
    h = F.conv2d(z, *p("conv_in"), padding=1)
    h = res("mid.block_2", attn("mid.attn_1", res("mid.block_1", h)))
    for i in reversed(range(levels)):
        for j in range(dd["num_res_blocks"] + 1):
            h = res(f"up.{i}.block.{j}", h)
            if res_h in dd["attn_resolutions"]:
                h = attn(f"up.{i}.attn.{j}", h)
        if i:
            h, res_h = conv3x3(h, *p(f"up.{i}.upsample.conv"), up=True), res_h * 2
    return conv3x3(h, *p("conv_out"), norm=p("norm_out"))


def decode_code(state, cfg, codes, like):
    """GumbelVQ.decode_code: codebook rows -> post_quant_conv -> Decoder, in the dtype / on the device of `like`."""
    z = state["quantize.embed.weight"].to(like)[codes.to(like.device)].permute(0, 3, 1, 2)
    z = F.conv2d(z, state["post_quant_conv.weight"].to(like), state["post_quant_conv.bias"].to(like))
    return decoder(state, cfg["ddconfig"], z)


def rel(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm())
