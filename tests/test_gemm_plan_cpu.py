"""CPU: which kernel every named product launches -- the GEMM planner's decisions (ofa_gemm_plan, host only) pinned in one table.

A change that moves a product to another kernel, tile, K-split or launch shows up here, not as a step-time change on a GPU box."""
import ctypes

import pytest

from ofasys_amd import lib as L

NT, NN, TN, TT = (0, 1), (0, 0), (1, 0), (1, 1)
ACCUM, OUT_F32, A_KPAD_ZERO, DEFER_REDUCE = 4, 16, 32, 128
WS = 256 << 20                  # the step's GEMM workspace (kernels.workspace)
R, RD = 13312, 1536             # encoder / decoder rows of the packed cfg-2 batch (tools/gemm_bench.py)
KERNELS = ("SIMPLE", "REG", "LDS_DMA", "RING", "BIG", "PP", "MIXED")
PLAN_LEN = 15


def plan(M, N, K, layout, flags=0, dtype=L.BF16, batch=1, ws=WS):
    p = (ctypes.c_int * PLAN_LEN)()
    L.lib().call("ofa_gemm_plan", M, N, K, layout[0], layout[1], batch, flags, dtype, ws, ctypes.addressof(p))
    return list(p)


def describe(p):
    """One line per plan; every field of ofa_gemm_plan is either in it or implied by it (asserted)."""
    kernel, why, wm, wn, tm, tn, bm, bn, splits, ksplit, k, tall, short, colstat, reduce = p
    if KERNELS[kernel] == "SIMPLE":
        assert p[2:] == [0] * (PLAN_LEN - 2)
        return f"SIMPLE why={why}"
    assert why == 0 and (bm, bn) == (32 * tm * wm, 32 * tn * wn)
    assert (tall > 0 and short > 0) == (KERNELS[kernel] == "MIXED") and reduce <= (splits > 1)
    s = f"{KERNELS[kernel]} {bm}x{bn} waves {wm}x{wn} of {tm}x{tn} K={k}"
    if splits > 1:
        s += f" splits={splits}x{ksplit}" + (" +reduce" if reduce else "")
    else:
        assert ksplit == k
    if tall:
        s += f" rows={tall}+{short}"
    return s + f" colstat={colstat}"


# name -> (M, N, K, layout, flags, dtype, batch, workspace)
PRODUCTS = {
    # the cfg-2 step's products (tools/gemm_bench.py, profiles/round6_gemm_microbench.txt)
    "qkv forward": (R, 2304, 768, NT, 0, L.BF16, 1, WS),
    "out_proj forward": (R, 768, 768, NT, 0, L.BF16, 1, WS),
    "fc1 forward": (R, 3072, 768, NT, 0, L.BF16, 1, WS),
    "fc2 forward": (R, 768, 3072, NT, 0, L.BF16, 1, WS),
    "cross k|v of 6 layers": (R, 9216, 768, NT, 0, L.BF16, 1, WS),
    "decoder qkv": (RD, 2304, 768, NT, 0, L.BF16, 1, WS),
    "decoder fc1": (RD, 3072, 768, NT, 0, L.BF16, 1, WS),
    "decoder fc2": (RD, 768, 3072, NT, 0, L.BF16, 1, WS),
    "output projection": (RD, 51272, 768, NT, 0, L.BF16, 1, WS),
    "qkv dgrad": (R, 768, 2304, NN, 0, L.BF16, 1, WS),
    "out_proj dgrad": (R, 768, 768, NN, 0, L.BF16, 1, WS),
    "fc1 dgrad": (R, 768, 3072, NN, 0, L.BF16, 1, WS),
    "fc2 dgrad": (R, 3072, 768, NN, 0, L.BF16, 1, WS),
    "output projection dgrad (padded logit gradient)": (RD, 768, 51328, NN, A_KPAD_ZERO, L.BF16, 1, WS),
    "embedding / output weight gradient": (51272, 768, RD, TN, ACCUM, L.BF16, 1, WS),
    "embedding / output weight gradient, fp32, deferred": (51272, 768, RD, TN, ACCUM | OUT_F32 | DEFER_REDUCE, L.BF16, 1, WS),
    "large square": (8192, 8192, 8192, NT, 0, L.BF16, 1, WS),
    # shapes the planner's comments cite as measured
    "fc2 dgrad as 13312 x 3072 x 768 NN": (13312, 3072, 768, NN, 0, L.BF16, 1, WS),
    "2048 x 2304 x 768": (2048, 2304, 768, NT, 0, L.BF16, 1, WS),
    "1536 x 768 x 3072 dgrad": (1536, 768, 3072, NN, 0, L.BF16, 1, WS),
    "18432 x 256 x 1024": (18432, 256, 1024, NT, 0, L.BF16, 1, WS),
    "6272 x 256 x 1024": (6272, 256, 1024, NT, 0, L.BF16, 1, WS),
    "18432 x 256 x 2304": (18432, 256, 2304, NT, 0, L.BF16, 1, WS),
    "13312 x 768 x 3072 NT": (13312, 768, 3072, NT, 0, L.BF16, 1, WS),
    "13312 x 9216 x 768 NN": (13312, 9216, 768, NN, 0, L.BF16, 1, WS),
    # fp16, no workspace, batched, fp32 output / accumulation
    "fc1 forward f16": (R, 3072, 768, NT, 0, L.F16, 1, WS),
    "fc1 dgrad f16": (R, 768, 3072, NN, 0, L.F16, 1, WS),
    "decoder fc2 f16, no workspace": (RD, 768, 3072, NT, 0, L.F16, 1, 0),
    "decoder fc2, no workspace": (RD, 768, 3072, NT, 0, L.BF16, 1, 0),
    "output projection dgrad, no workspace": (RD, 768, 51328, NN, A_KPAD_ZERO, L.BF16, 1, 0),
    "weight gradient 768 x 768 over 13312 rows": (768, 768, R, TN, 0, L.BF16, 1, WS),
    "weight gradient 768 x 768 over 13312 rows, no workspace": (768, 768, R, TN, 0, L.BF16, 1, 0),
    "weight gradient 3072 x 768 over 1000 rows": (3072, 768, 1000, TN, 0, L.BF16, 1, WS),
    "qkv forward, fp32 output": (R, 2304, 768, NT, OUT_F32, L.BF16, 1, WS),
    "fc1 dgrad, accumulate": (R, 768, 3072, NN, ACCUM, L.BF16, 1, WS),
    "attention-sized batch of 96": (256, 256, 64, NT, 0, L.BF16, 96, WS),
    "batch of 3 decoder fc1": (RD, 3072, 768, NT, 0, L.BF16, 3, WS),
    "batch of 3 fc2 dgrad": (2048, 3072, 768, NN, 0, L.BF16, 3, WS),
    "batch of 4 weight gradients": (768, 768, 2048, TN, 0, L.F16, 4, WS),
    "TT layout": (1024, 1024, 1024, TT, 0, L.BF16, 1, WS),
    "register-staged ragged K": (2048, 2048, 1000, NN, 0, L.BF16, 1, WS),
    # the exact kernel
    "fp32 operands": (R, 768, 768, NT, 0, L.F32, 1, WS),
    "forced simple": (R, 768, 768, NT, 8, L.BF16, 1, WS),
    "ragged K on a k-major B": (100, 100, 100, NT, 0, L.BF16, 1, WS),
}

EXPECTED = {
    'qkv forward': 'BIG 256x256 waves 2x4 of 4x2 K=768 colstat=128',
    'out_proj forward': 'BIG 192x256 waves 2x4 of 3x2 K=768 colstat=96',
    'fc1 forward': 'MIXED 256x256 waves 2x4 of 4x2 K=768 rows=16+48 colstat=128',
    'fc2 forward': 'BIG 192x256 waves 2x4 of 3x2 K=3072 colstat=96',
    'cross k|v of 6 layers': 'BIG 256x256 waves 2x4 of 4x2 K=768 colstat=128',
    'decoder qkv': 'LDS_DMA 64x128 waves 1x2 of 2x2 K=768 colstat=64',
    'decoder fc1': 'LDS_DMA 64x128 waves 1x2 of 2x2 K=768 colstat=64',
    'decoder fc2': 'RING 64x64 waves 2x2 of 1x1 K=3072 colstat=32',
    'output projection': 'BIG 256x256 waves 2x4 of 4x2 K=768 colstat=128',
    'qkv dgrad': 'PP 192x256 waves 2x4 of 3x2 K=2304 colstat=96',
    'out_proj dgrad': 'BIG 192x256 waves 2x4 of 3x2 K=768 colstat=96',
    'fc1 dgrad': 'PP 192x256 waves 2x4 of 3x2 K=3072 colstat=96',
    'fc2 dgrad': 'MIXED 256x256 waves 2x4 of 4x2 K=768 rows=16+48 colstat=64',
    'output projection dgrad (padded logit gradient)': 'PP 256x256 waves 2x4 of 4x2 K=51328 splits=14x3712 +reduce colstat=0',
    'embedding / output weight gradient': 'PP 256x256 waves 2x4 of 4x2 K=1536 colstat=128',
    'embedding / output weight gradient, fp32, deferred': 'BIG 256x256 waves 2x4 of 4x2 K=1536 colstat=128',
    'large square': 'BIG 256x256 waves 2x4 of 4x2 K=8192 colstat=128',
    'fc2 dgrad as 13312 x 3072 x 768 NN': 'MIXED 256x256 waves 2x4 of 4x2 K=768 rows=16+48 colstat=64',
    '2048 x 2304 x 768': 'LDS_DMA 64x128 waves 1x2 of 2x2 K=768 colstat=64',
    '1536 x 768 x 3072 dgrad': 'RING 64x64 waves 2x2 of 1x1 K=3072 colstat=32',
    '18432 x 256 x 1024': 'LDS_DMA 64x128 waves 1x2 of 2x2 K=1024 colstat=64',
    '6272 x 256 x 1024': 'RING 64x64 waves 2x2 of 1x1 K=1024 colstat=32',
    '18432 x 256 x 2304': 'LDS_DMA 64x128 waves 1x2 of 2x2 K=2304 colstat=64',
    '13312 x 768 x 3072 NT': 'BIG 192x256 waves 2x4 of 3x2 K=3072 colstat=96',
    '13312 x 9216 x 768 NN': 'BIG 256x256 waves 2x4 of 4x2 K=768 colstat=128',
    'fc1 forward f16': 'MIXED 256x256 waves 2x4 of 4x2 K=768 rows=16+48 colstat=128',
    'fc1 dgrad f16': 'PP 192x256 waves 2x4 of 3x2 K=3072 colstat=96',
    'decoder fc2 f16, no workspace': 'RING 64x64 waves 2x2 of 1x1 K=3072 colstat=32',
    'decoder fc2, no workspace': 'RING 64x64 waves 2x2 of 1x1 K=3072 colstat=32',
    'output projection dgrad, no workspace': 'RING 64x64 waves 2x2 of 1x1 K=51328 colstat=32',
    'weight gradient 768 x 768 over 13312 rows': 'LDS_DMA 128x128 waves 2x2 of 2x2 K=13312 splits=11x1216 +reduce colstat=0',
    'weight gradient 768 x 768 over 13312 rows, no workspace': 'RING 64x64 waves 2x2 of 1x1 K=13312 colstat=32',
    'weight gradient 3072 x 768 over 1000 rows': 'LDS_DMA 64x64 waves 1x1 of 2x2 K=1024 colstat=64',
    'qkv forward, fp32 output': 'BIG 256x256 waves 2x4 of 4x2 K=768 colstat=128',
    'fc1 dgrad, accumulate': 'PP 192x256 waves 2x4 of 3x2 K=3072 colstat=96',
    'attention-sized batch of 96': 'LDS_DMA 128x128 waves 2x2 of 2x2 K=64 colstat=0',
    'batch of 3 decoder fc1': 'LDS_DMA 128x128 waves 2x2 of 2x2 K=768 colstat=0',
    'batch of 3 fc2 dgrad': 'LDS_DMA 128x128 waves 2x2 of 2x2 K=768 colstat=0',
    'batch of 4 weight gradients': 'LDS_DMA 128x128 waves 2x2 of 2x2 K=2048 splits=3x704 +reduce colstat=0',
    'TT layout': 'RING 64x64 waves 2x2 of 1x1 K=1024 colstat=32',
    'register-staged ragged K': 'REG 64x128 waves 1x2 of 2x2 K=1000 colstat=64',
    'fp32 operands': 'SIMPLE why=1',
    'forced simple': 'SIMPLE why=2',
    'ragged K on a k-major B': 'SIMPLE why=3',
}


@pytest.mark.parametrize("name", sorted(PRODUCTS))
def test_gemm_plan_table(name):
    M, N, K, layout, flags, dtype, batch, ws = PRODUCTS[name]
    assert describe(plan(M, N, K, layout, flags, dtype, batch, ws)) == EXPECTED[name]


def test_gemm_plan_agrees_with_splits_and_rejects_bad_arguments():
    for M, N, K, layout, flags, dtype, batch, ws in PRODUCTS.values():
        p = plan(M, N, K, layout, flags, dtype, batch, ws)
        if p[0]:                                                   # (ofa_gemm_splits: 1 for the exact kernel)
            assert L.lib().cdll.ofa_gemm_splits(M, N, K, layout[0], layout[1], batch, flags, dtype, ws) == p[8]
    with pytest.raises(L.OfaError, match="gemm_plan"):
        plan(0, 768, 768, NT)
    with pytest.raises(L.OfaError, match="gemm_plan"):
        plan(768, 768, 768, NT, dtype=7)
