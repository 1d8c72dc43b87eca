"""The VQGAN encoder tests' shared cases and their float64 restatement (tests/test_vqgan_encode_cpu.py, tests/test_vqgan_encode_gpu.py,
tools/vqgan_bench.py).  TEST INFRASTRUCTURE in the style of tests/vqgan_case.py: plain torch on NCHW maps, written from the formulas --
taming's Downsample (zero pad on the bottom and right, 3 x 3 at stride 2), conv_in, the Encoder, and the Gumbel quantizer's
argmax_n (proj(h)[n] + g[n]) -- and nothing of the kernels, in the dtype and on the device of the input.  Exact cases follow vqgan_case."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import vqgan_case as C
from tests.stream_oracle import philox4x32_10


def downsample(x, w, b):
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)


def down_cases(plan):
    """[(id, H, W, C)] (the SOURCE map's; B = 2) from plan(C) -> (tile rows, tile columns, Cin slice, channel block, lds)."""
    th, tw = plan(32)[:2]
    one = max(c for c in range(32, 513, 32) if plan(c)[2] == c)           # the largest C that is ONE slice
    blocks = 2 * plan(512)[3]                                             # two whole channel blocks of the widest kernel
    assert plan(one + 32)[2] < one + 32 and plan(blocks)[3] < blocks
    maps = ((2, 2), (5, 4), (4, 5), (2 * th - 2, 2 * tw + 2), (2 * th + 3, 2 * tw - 1))
    return [(f"{h}x{w}", h, w, 32) for h, w in maps] + [(f"c{c}", 6, 7, c) for c in (one, one + 32, blocks)]


def exact_down(case, seed=0):
    _, H, W, Cn = case
    gen = torch.Generator().manual_seed(seed)
    t = dict(x=C.ints(gen, 2, Cn, H, W), b=C.ints(gen, Cn))
    t["w"] = C.ints(gen, Cn, Cn, 3, 3, hi=1) * (torch.rand(Cn, Cn, 3, 3, generator=gen) < 0.125)
    t["want"] = downsample(t["x"], t["w"], t["b"])
    assert torch.equal(t["want"], t["want"].round()) and float(t["want"].abs().max()) <= 256, "change the seed, not the bound"
    return t


def exact_conv_in(H, W, Cout, seed=0):
    gen = torch.Generator().manual_seed(seed)
    t = dict(x=C.ints(gen, 2, 3, H, W), w=C.ints(gen, Cout, 3, 3, 3, hi=1), b=C.ints(gen, Cout))
    t["want"] = F.conv2d(t["x"], t["w"], t["b"], padding=1)
    return t


def exact_logits(N, K, n_embed, seed=0):
    """h [N, K], w [n_embed, K], b [n_embed] (float64 integers) and their logits [N, n_embed]: small integers, so ties are everywhere."""
    gen = torch.Generator().manual_seed(seed)
    t = dict(h=C.ints(gen, N, K), b=C.ints(gen, n_embed), w=C.ints(gen, n_embed, K, hi=1) * (torch.rand(n_embed, K, generator=gen) < 0.125))
    t["logits"] = t["h"] @ t["w"].T + t["b"]
    assert float(t["logits"].abs().max()) <= 256
    return t


def column_logits(cols, N):
    """Designed logits: row r of h is the unit vector of column r % K, so logits[r] = cols[:, r % K] exactly.  cols [n_embed, K]."""
    K = cols.shape[1]
    return dict(h=torch.eye(K, dtype=torch.float64)[torch.arange(N) % K], w=cols.double(), logits=cols.double().T[torch.arange(N) % K])


def planted(n_embed, K, second_split):
    """cols [n_embed, K] and the wanted code per column: see test_quantize_planted."""
    gen = torch.Generator().manual_seed(5)
    cols, bias = torch.randint(-3, 4, (n_embed, K), generator=gen).double(), torch.zeros(n_embed, dtype=torch.float64)
    want = torch.full((K,), -1, dtype=torch.int64)
    cols[0, 0], cols[n_embed - 1, 1], want[0], want[1] = 6, 6, 0, n_embed - 1         # the first and the last code
    cols[:, 2] = torch.randint(-9, -3, (n_embed,), generator=gen).double()             # every logit negative
    cols[17, 2], want[2] = -2, 17
    cols[:, 3], bias[37], want[3] = 4, 1, 37                                            # the bias alone decides
    for k, (lo, hi) in {4: (1, 5), 5: (3, 64 + 3), 6: (10, second_split + 10)}.items():   # lane halves, waves, splits: the lowest index
        cols[lo, k], cols[hi, k], want[k] = 7, 7, lo
    return cols, bias, want


def gumbel(N, n_embed, seed):
    """float64 g [N, n_embed]: -log(-log(u)), u = ((word >> 8) + 0.5) 2^-24, word n % 4 of Philox(counter r n_embed / 4 + n / 4, key seed)."""
    ctr = (np.arange(N, dtype=np.uint64)[:, None] * np.uint64(n_embed // 4) + np.arange(n_embed // 4, dtype=np.uint64)[None, :]).reshape(-1)
    zero = np.zeros_like(ctr)
    words = philox4x32_10((ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), zero, zero), (seed & 0xFFFFFFFF, seed >> 32))
    u = ((np.stack(words, axis=1).reshape(N, n_embed) >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    return torch.from_numpy(-np.log(-np.log(u)))


def decided(scores, gap=1e-3):
    """(float64 arg-max, mask of the rows whose top-two gap is at least `gap`)."""
    top = scores.topk(2, dim=1).values
    return scores.argmax(1), (top[:, 0] - top[:, 1]) >= gap


def encoder(state, dd, x, prefix="encoder."):
    """taming's Encoder on x NCHW from a reference-keyed state dict, in x's dtype on x's device."""
    p = lambda name: (state[prefix + name + ".weight"].to(x), state[prefix + name + ".bias"].to(x))      # noqa: E731

    def res(name, x):
        h = C.conv3x3(x, *p(name + ".conv1"), norm=p(name + ".norm1"))
        skip = F.conv2d(x, *p(name + ".nin_shortcut")) if prefix + name + ".nin_shortcut.weight" in state else x
        return C.conv3x3(h, *p(name + ".conv2"), norm=p(name + ".norm2"), res=skip)

    def attn(name, x):
        B, Cn, H, W = x.shape
        h = F.group_norm(x, 32, *p(name + ".norm"), eps=1e-6)
        q, k, v = (F.conv2d(h, *p(f"{name}.{n}")).reshape(B, Cn, H * W) for n in "qkv")
        a = torch.softmax(torch.bmm(q.transpose(1, 2), k) * Cn ** -0.5, dim=2)
        return x + F.conv2d(torch.bmm(v, a.transpose(1, 2)).reshape(B, Cn, H, W), *p(name + ".proj_out"))

    levels, side = len(dd["ch_mult"]), x.shape[2]
    h = F.conv2d(x, *p("conv_in"), padding=1)
    for i in range(levels):
        for j in range(dd["num_res_blocks"]):
            h = res(f"down.{i}.block.{j}", h)
            if side in dd["attn_resolutions"]:
                h = attn(f"down.{i}.attn.{j}", h)
        if i != levels - 1:
            h, side = downsample(h, *p(f"down.{i}.downsample.conv")), side // 2
    h = res("mid.block_2", attn("mid.attn_1", res("mid.block_1", h)))
    return C.conv3x3(h, *p("conv_out"), norm=p("norm_out"))


def prequant(state, cfg, x):
    """GumbelVQ.encode_to_prequant: quant_conv(Encoder(x)), in x's dtype."""
    return F.conv2d(encoder(state, cfg["ddconfig"], x), state["quant_conv.weight"].to(x), state["quant_conv.bias"].to(x))
