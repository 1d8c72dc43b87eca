"""CPU: register-allocation guard for the hot kernels.  hipcc cross-compiles gfx950 here; a kernel that starts spilling
(e.g. the GELU+LayerNorm backward at its 128-VGPR cap: 73 us -> 195 us per call when an innocent-looking change added
16 registers) is a silent 10% step-time regression, so the spill counts in the code-object metadata are pinned."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ofasys_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


_CACHE = {}


def _kernel_meta(src, tmp_path):
    if src in _CACHE:
        return _CACHE[src]
    out = tmp_path / (src + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", os.path.join(CSRC, src),
                    "-o", str(out)], check=True, stderr=subprocess.DEVNULL)
    meta = {}
    for blk in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                      for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    _CACHE[src] = meta
    return meta


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("src,pattern,max_spill", [
    ("layernorm.hip", r"ln_bwd_kernelItLi1ELi8ELb1E", 8),       # GELU + LayerNorm backward of the 4D FFN rows (bf16)
    ("layernorm.hip", r"ln_bwd_kernelItLi2ELi1ELb0E", 0),       # LayerNorm backward, D = 768 rows (bf16)
    ("attention.hip", r"attn_(fwd|bwd_dkv)(_f16)?_lds_kernel", 0),          # bias-free attention: three / two waves per SIMD, no spills
    # dQ runs THREE waves per SIMD (168 registers): the 3 registers it spills there were measured worth it (backward 156 -> 145 us
    # at 448 x 448 against two waves without spills, profiles/round2_attention_timeline.txt)
    ("attention.hip", r"attn_bwd_dq(_f16)?_lds_kernel", 4),
    # the shared position bias: forward at three waves per SIMD (the bias image is the score MFMAs' initial accumulator: 8 staging
    # registers), dQ at two waves without spills, dK/dV with the image staged through LDS (was 16 spilled registers with it in registers)
    ("attention.hip", r"attn_fwd_sbias(_f16)?_lds_kernel", 2),
    ("attention.hip", r"attn_bwd_dq_sbias(_f16)?_lds_kernel", 0),
    ("attention.hip", r"attn_bwd_dkv_sbias_lds_kernel", 6),
    ("attention.hip", r"attn_bwd_dkv_sbias_f16_lds_kernel", 18),          # (the fp16 decode holds more temporaries; 10 before the column-sum epilogue of round 6)
    ("gemm_mfma.hip", r"gemm_mfma_kernelILi2ELi2ELb[01]ELb[01]ELb0ELb1E", 0),   # 128x128 LDS-DMA kernels, bf16 out
    ("gemm_mfma.hip", r"gemm_ring_kernelILi[12]ELi[12]ELb[01]ELb[01]ELb0E", 0),  # 4-stage ring kernels, bf16 out
    ("gemm_mfma.hip", r"gemm_group_tn_kernel", 0),                               # grouped weight gradients (256 accumulator registers live)
    ("gemm_mfma.hip", r"gemm_big_mixed_kernel", 0),                              # 256- and 192-row tiles in one launch (round 6): both bodies in one kernel
    # the ping-pong loop (round 5): 128 accumulator + 48 fragment registers per wave, two waves per SIMD -- a spilled register inside its
    # load / MFMA segments would also put scratch traffic on the vmcnt counter the loop's LDS-DMA waits are counted on
    ("gemm_pp.hip", r"gemm_pp_kernel", 0),
    ("gemm_pp.hip", r"gemm_group_tn_pp_kernel", 0),
    # the one-pass SCST loss row: the row's NV x 4 registers at two blocks of 1024 threads per CU (64 registers), every NV, bf16 and fp16
    ("loss_optim.hip", r"scst_fwd_grad_kernel", 0),
])
def test_hot_kernels_do_not_spill(tmp_path, src, pattern, max_spill):
    meta = _kernel_meta(src, tmp_path)
    hits = {k: v for k, v in meta.items() if re.search(pattern, k)}
    assert hits, f"no kernel matching {pattern} in {src}"
    for k, v in hits.items():
        assert v["vgpr_spill_count"] <= max_spill, (k, v)
        if src == "gemm_pp.hip":
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= 256, (k, v)
